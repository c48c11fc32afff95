"""SIGNS, STEPPED of include/gq_drive.h and include/gq_eden.h restated in Python integers, nothing else: the four sign words of a
launch at (seed, step).  The expected outputs of every stepped launch are tests/drive_contract.py's / tests/eden_contract.py's given
these words (tests/test_rot_step_contract.py checks this restatement on the CPU, tests/test_gpu_zz_rot_step_contract.py holds the
kernels to it)."""

M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


def step_words(seed, step):
    """Word k = 0 ... 3: z = seed + (4 * step + k + 1) * GAMMA mod 2^64, then splitmix64's finaliser."""
    words = []
    for k in range(4):
        z = (seed + (4 * step + k + 1) * GAMMA) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        words.append(z ^ (z >> 31))
    return tuple(words)
