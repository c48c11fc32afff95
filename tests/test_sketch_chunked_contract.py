"""The README's recovery-error table without a GPU: the setting of tools/sketch_recovery.py on the restatements, `global`
(tests/sketch_contract.py) next to `chunked` (tests/sketch_chunked_contract.py).  The README must carry the figures computed here."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sketch_recovery  # noqa: E402


def test_recovery_error_table_is_the_readmes():
    t = sketch_recovery.tables()
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    for name, label in (("global", ""), ("chunked", ", chunked")):
        for R in (1, 8):
            line = "| R = %d%s | %s |" % (R, label, " | ".join("%.3f" % t[name]["R%d_rows%d" % (R, rows)] for rows in (1, 3, 5)))
            assert line in readme, line
