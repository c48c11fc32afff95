"""include/gq_sketch.h restated in numpy, one float32 operation at a time: the hash, the window lists, the two-level sums, the median
network and the decode-mean with top-k's kept set (tests/topk_contract.py).  tests/test_sketch_contract.py checks it against float64 /
brute force; the GPU tests compare the kernels with it bit for bit."""
import numpy as np

import topk_contract as tc

CHUNK, UNIT, HEADER = 4096, 8, 16
G, M = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xD6E8FEB86659FD93)
f32, u32, u64 = np.float32, np.uint32, np.uint64


def fin(z):
    z = np.atleast_1d(np.asarray(z, u64)).copy()
    z = (z ^ (z >> u64(30))) * u64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> u64(27))) * u64(0x94D049BB133111EB)
    return z ^ (z >> u64(31))


def layout(n, rows, C):
    items = -(-n // CHUNK)
    return items, max(1, -(-items // (C * rows)))


def sketched(n, rows, C):
    items, nwin = layout(n, rows, C)
    return 2 * rows * nwin <= items


def section_bytes(n, rows, C):
    items, nwin = layout(n, rows, C)
    return HEADER + 4 * CHUNK * rows * nwin if sketched(n, rows, C) else 4 * n


def row(seed, j):
    """-> (K_j, A_j)"""
    key = fin(np.array([seed], u64) + np.array([j + 1], u64) * G)[0]
    return key, int((key >> u64(20)) & u64(0xfff)) | 1


def item_hash(key, items, nwin):
    """-> (window, off) of the items 0 .. items - 1"""
    h = fin(key + (np.arange(items, dtype=u64) + u64(1)) * G)
    return (((h >> u64(32)) * u64(nwin)) >> u64(32)).astype(np.int64), (h & u64(0xfff)).astype(np.int64)


def cells(A, off):
    return (A * np.arange(CHUNK, dtype=np.int64) + off) & (CHUNK - 1)


def signs(key, a):
    """bit t of item a's 4,096 sign bits"""
    w = fin(key + ((u64(a) << u64(6)) + np.arange(64, dtype=u64) + u64(1)) * M)
    t = np.arange(CHUNK, dtype=u64)
    return ((w[(t >> u64(6)).astype(np.int64)] >> (t & u64(63))) & u64(1)).astype(u32)


def lists(seed, rows, items, nwin):
    """[row][window] -> the ascending items"""
    out = []
    for j in range(rows):
        win, _ = item_hash(row(seed, j)[0], items, nwin)
        out.append([np.flatnonzero(win == v) for v in range(nwin)])
    return out


def sketch(w, seed, rows, nwin):
    """-> float32 [rows, nwin, 4096]: the chunks' partial sums from +0 in list order, the partials from +0 in chunk order"""
    w = tc.f32(w)
    items = -(-w.size // CHUNK)
    x = np.zeros(items * CHUNK, f32)
    x[:w.size] = w
    xb = x.view(u32).reshape(items, CHUNK)
    T = np.zeros((rows, nwin, CHUNK), f32)
    for j in range(rows):
        key, A = row(seed, j)
        win, off = item_hash(key, items, nwin)
        for v in range(nwin):
            lst = np.flatnonzero(win == v)
            total = np.zeros(CHUNK, f32)
            for c in range(0, len(lst), UNIT):
                part = np.zeros(CHUNK, f32)
                for a in lst[c:c + UNIT]:
                    term = np.empty(CHUNK, f32)
                    term[cells(A, off[a])] = (xb[a] ^ (signs(key, a) << u32(31))).view(f32)
                    with np.errstate(invalid="ignore", over="ignore"):
                        part = (part + term).astype(f32)
                with np.errstate(invalid="ignore", over="ignore"):
                    total = (total + part).astype(f32)
            T[j, v] = total
    return T


def section(w, seed, rows, C):
    n = tc.f32(w).size
    nwin = layout(n, rows, C)[1]
    return np.concatenate([np.array([n, rows, nwin, 0], u32).view(np.uint8), sketch(w, seed, rows, nwin).reshape(-1).view(np.uint8)])


def tables(sec):
    sec = np.ascontiguousarray(sec, np.uint8)
    n, rows, nwin, _ = (int(x) for x in sec[:HEADER].view(u32))
    return sec[HEADER:].view(f32).reshape(rows, nwin, CHUNK)


def cx(x, y):
    swap = y < x
    return np.where(swap, y, x), np.where(swap, x, y)


def median(p):
    """p: [rows, ...] -> the header's network"""
    p = [a for a in p]
    net = {1: [], 3: [(0, 1), (1, 2), (0, 1)], 5: [(0, 1), (3, 4), (0, 3), (1, 4), (1, 2), (2, 3), (1, 2)]}[len(p)]
    with np.errstate(invalid="ignore"):
        for a, b in net:
            p[a], p[b] = cx(p[a], p[b])
    return p[len(p) // 2]


def mean_table(payloads, E=None):
    """payloads: R tables -> T"""
    acc = np.zeros_like(payloads[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for t in payloads:
            acc = (acc + t).astype(f32)
        T = (acc / f32(len(payloads))).astype(f32)
        if E is not None:
            T = (T + E.reshape(T.shape)).astype(f32)
    return T


def estimates(T, n, seed):
    rows, nwin, _ = T.shape
    items = -(-n // CHUNK)
    vals = np.empty((rows, items, CHUNK), f32)
    for j in range(rows):
        key, A = row(seed, j)
        win, off = item_hash(key, items, nwin)
        for a in range(items):
            vals[j, a] = (T[j, win[a], cells(A, off[a])].view(u32) ^ (signs(key, a) << u32(31))).view(f32)
    return median(vals).reshape(-1)[:n]


def decode_mean(payloads, n, k, seed, E=None):
    """-> (out, the new E or None)"""
    T = mean_table(payloads, E)
    est = estimates(T, n, seed)
    out = np.zeros(n, f32)
    idx = tc.kept(est, k)
    out[idx] = est[idx]
    if E is None:
        return out, None
    with np.errstate(invalid="ignore", over="ignore"):
        return out, (T - sketch(out, seed, T.shape[0], T.shape[1])).astype(f32).reshape(-1)
