"""include/gq_psgd.h restated in numpy: every float32 operation one at a time (fmaf as tests/kmeans_contract.py restates it, the
counter hash as tests/qsgd_contract.py does), the reductions in the header's trees.  Builds wires and steps the warm start over
records; `mut` names ONE deliberate departure from the header (the mutation checks: each must change bits).  Also the independent
float64 witness the restatement itself is held to."""
import numpy as np

from kmeans_contract import fmaf
from qsgd_contract import uniform_bits

f32, u32, f64 = np.float32, np.uint32, np.float64
PIECE, ROW_BLOCK, TILE_COLS, HEADER = 4096, 64, 256, 16
EPS = f32(1e-8)
SERVER_USER = 4095
U = 2.0 ** -24          # float32's unit roundoff


def section_nbytes(n, m, r):
    return (HEADER + 4 * r * (n + m) + 15) // 16 * 16


def matrix_of(shape):
    """(n, m) of a tensor's matrix, or None for a vector / scalar."""
    if len(shape) < 2:
        return None
    n = int(shape[0])
    return n, int(np.prod(shape)) // n


def compresses(shape, r):
    nm = matrix_of(shape)
    numel = int(np.prod(shape))
    return nm is not None and numel > 1000 and min(nm) >= r and section_nbytes(nm[0], nm[1], r) < 4 * numel


def q0(seed, param, user, m, r):
    idx = np.uint64(((param << 12) | user) << 32) | np.arange(m * r, dtype=np.uint64)
    u = (uniform_bits(seed, idx) >> np.uint64(8)).astype(f32) * f32(U)
    return (f32(2.0) * u - f32(1.0)).astype(f32).reshape(m, r)


def _mac(a, b, x, mut):
    if mut == "unfused":
        with np.errstate(all="ignore"):
            return ((a * b).astype(f32) + x).astype(f32)
    with np.errstate(all="ignore"):
        return fmaf(a, b, x)


def tree(x):
    """tree(x) over the last axis (256 values)."""
    with np.errstate(all="ignore"):
        for h in (128, 64, 32, 16, 8, 4, 2, 1):
            x = (x[..., :h] + x[..., h:2 * h]).astype(f32)
    return x[..., 0]


def dot(a, b, mut=None):
    """dot(a, b) over the last axis: 256 strided accumulators, ascending, then the tree."""
    a, b = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32))
    L = a.shape[-1]
    steps = max(1, -(-L // 256))
    pad = steps * 256 - L
    if pad:
        z = np.zeros(a.shape[:-1] + (pad,), f32)
        a, b = np.concatenate([a, z], -1), np.concatenate([b, z], -1)
    a, b = a.reshape(a.shape[:-1] + (steps, 256)), b.reshape(b.shape[:-1] + (steps, 256))
    valid = (np.arange(steps * 256) < L).reshape(steps, 256)
    x = np.zeros(a.shape[:-2] + (256,), f32)
    order = range(steps - 1, -1, -1) if mut == "reversed" else range(steps)
    for s in order:
        x = np.where(valid[s], _mac(a[..., s, :], b[..., s, :], x, mut), x)
    return tree(x)


def project(M, Q, mut=None):
    """P = M Q in the header's order: [n, r]."""
    n, m = M.shape
    P = None
    for c0 in range(0, m, PIECE) if m > PIECE else [0]:
        c1 = min(m, c0 + PIECE) if m > PIECE else m
        pp = dot(M[:, None, c0:c1], Q[c0:c1].T[None, :, :], mut)
        with np.errstate(all="ignore"):
            P = pp if P is None else (P + pp).astype(f32)
    return P


def orthogonalise(P, mut=None):
    """Modified Gram-Schmidt of the header -> (Ph, reset flags)."""
    P = P.copy()
    n, r = P.shape
    orig = P.copy()
    reset = np.zeros(r, bool)
    with np.errstate(all="ignore"):
        for j in range(r):
            for k in range(j):
                d = dot(P[:, k], orig[:, j] if mut == "classical" else P[:, j], mut)
                P[:, j] = _mac(-d, P[:, k], P[:, j], mut)
            nrm = np.sqrt(dot(P[:, j], P[:, j], mut), dtype=f32)
            P[:, j] = (P[:, j] / (nrm + EPS).astype(f32)).astype(f32)
            reset[j] = (nrm == 0) or not np.isfinite(nrm)
    return P, reset


def back_project(M, Ph, mut=None):
    """Q' = M^T Ph in the header's order: [m, r]."""
    n, m = M.shape
    r = Ph.shape[1]
    nb = -(-n // ROW_BLOCK)
    acc = np.zeros((nb, m, r), f32)
    rows = range(ROW_BLOCK - 1, -1, -1) if mut == "reversed" else range(ROW_BLOCK)
    for rr in rows:
        i = np.arange(nb) * ROW_BLOCK + rr
        ok = i < n
        ii = np.where(ok, i, 0)
        y = _mac(M[ii][:, :, None], Ph[ii][:, None, :], acc, mut)
        acc = np.where(ok[:, None, None], y, acc)
    Qn = acc[0]
    with np.errstate(all="ignore"):
        for b in range(1, nb):
            Qn = (Qn + acc[b]).astype(f32)
    return Qn


def dense(Ph, Qn, mut=None):
    """D = Ph Q'^T in the header's order: [n, m]."""
    with np.errstate(all="ignore"):
        D = (Ph[:, 0][:, None] * Qn[:, 0][None, :]).astype(f32)
        for j in range(1, Ph.shape[1]):
            D = _mac(Ph[:, j][:, None], Qn[:, j][None, :], D, mut)
    return D


def section(Ph, Qn):
    n, r = Ph.shape
    m = Qn.shape[0]
    raw = np.array([n, m, r, 0], u32).tobytes() + np.ascontiguousarray(Ph, f32).tobytes() + np.ascontiguousarray(Qn, f32).tobytes()
    return np.frombuffer(raw + b"\0" * (section_nbytes(n, m, r) - len(raw)), np.uint8).copy()


def parse(sec, n, m, r):
    f = sec[HEADER:HEADER + 4 * r * (n + m)].view(f32)
    return f[:n * r].reshape(n, r), f[n * r:].reshape(m, r)


class Record(object):
    pass


def record(M, Q, Q0, e=None, s=None, mut=None):
    """One record of one tensor (M: [n, m]; Q: the warm start; Q0: where a reset column goes back to; e, s: error feedback).
    -> Record with section, Ph, Qn (Q' as on the wire), Q (the next warm start), reset, D, e (the next residual or None), Mp."""
    M = np.asarray(M, f32)
    with np.errstate(all="ignore"):
        Mp = M if e is None else (M + (f32(s) * e.reshape(M.shape)).astype(f32)).astype(f32)
    r = Q.shape[1]
    out = Record()
    out.Mp = Mp
    out.P = project(Mp, Q, mut)
    out.Ph, out.reset = orthogonalise(out.P, mut)
    out.Qn = back_project(Mp, out.Ph, mut)
    out.section = section(out.Ph, out.Qn)
    out.Q = np.where(out.reset[None, :], Q0, out.Qn).astype(f32)
    out.D = dense(out.Ph, out.Qn, mut)
    with np.errstate(all="ignore"):
        out.e = None if e is None else (Mp - out.D).astype(f32)
    assert out.Q.shape == (M.shape[1], r)
    return out


def decode_mean(sections, n, m, r):
    acc = None
    with np.errstate(all="ignore"):
        for sec in sections:
            D = dense(*parse(sec, n, m, r))
            acc = D if acc is None else (acc + D).astype(f32)
        return (acc / f32(len(sections))).astype(f32)


def same(a, b):
    """The header's equality: bit for bit on everything that is not a NaN, NaN where the other is NaN."""
    a, b = np.ascontiguousarray(a, f32).reshape(-1), np.ascontiguousarray(b, f32).reshape(-1)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u32)[~na], b.view(u32)[~nb]))


def same_section(a, b, n, m, r):
    """Two wire sections: header and padding byte for byte, the factors by `same`."""
    k = HEADER + 4 * r * (n + m)
    return (a.shape == b.shape and np.array_equal(a[:HEADER], b[:HEADER]) and np.array_equal(a[k:], b[k:])
            and same(a[HEADER:k].view(f32), b[HEADER:k].view(f32)))


# ---- the float64 witness: the same algorithm with numpy's own matrix products, nothing shared with the code above --------------
def witness(M, Q):
    """-> (Ph, Q', D) in float64: P = M Q, modified Gram-Schmidt with the epsilon, Q' = M^T Ph, D = Ph Q'^T."""
    M, Q = np.asarray(M, f64), np.asarray(Q, f64)
    P = M @ Q
    for j in range(P.shape[1]):
        for k in range(j):
            P[:, j] -= (P[:, k] @ P[:, j]) * P[:, k]
        P[:, j] /= np.sqrt(P[:, j] @ P[:, j]) + 1e-8
    Qn = M.T @ P
    return P, Qn, P @ Qn.T


def best_rank_error(M, r):
    """The Frobenius error of the best rank-r approximation (numpy's float64 SVD), and the singular values."""
    sv = np.linalg.svd(np.asarray(M, f64), compute_uv=False)
    return float(np.sqrt(np.sum(sv[r:] ** 2))), sv


def low_rank_plus_noise(n, m, r, seed, noise=1e-3):
    """U diag(sigma) V^T + noise with orthonormal U, V: sigma_1 ... sigma_r evenly from 2 down to 1 (1.5 at rank 1), the noise N(0, 1)
    entries times noise / sqrt(max(n, m)): its largest singular value is about noise * (1 + sqrt(min / max)), which the callers
    check against sigma_r with numpy's SVD."""
    rs = np.random.RandomState(seed)
    Uq, _ = np.linalg.qr(rs.standard_normal((n, r)))
    Vq, _ = np.linalg.qr(rs.standard_normal((m, r)))
    sig = np.linspace(2.0, 1.0, r) if r > 1 else np.array([1.5])
    A = (Uq * sig) @ Vq.T + noise * rs.standard_normal((n, m)) / np.sqrt(max(n, m))
    return A.astype(f32)


def specials(a, seed):
    """+-0, subnormals, +-inf and NaNs of both signs strewn into a copy of `a`."""
    rs = np.random.RandomState(seed)
    a = np.array(a, f32).copy()
    flat = a.reshape(-1)
    pos = rs.permutation(flat.size)[:12]
    flat[pos] = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc00000,
                          0xffc00000, 0x7f800001, 0xffffffff], u32).view(f32)
    return a
