"""The float32 model of vaeq_ldpc_sc_decode (include/vaeq.h): the sliding-window decoder of a spatially coupled LDPC chain, with the layer update of
tests/_ref_ldpc.py (every multiply, add and subtract a separately rounded numpy float32 operation in the order the header fixes).

decode()         one chain, vectorised over the Z checks of a layer, compressed messages (m1, m2, idx, signs), and the window kept as the kernel
                 keeps it: a ring of W + ms column-block slots for L and the TX bits (column block i in slot i mod (W + ms)), a ring of W
                 row-block slots for the check states (row block t in slot t mod W), blocks entering and leaving as the window moves;
decode_scalar()  an independent restatement: the dense coupled H, one explicit float32 message per edge, all L in one array, no ring and no
                 notion of entering or leaving -- tests/test_ref_ldpc_sc_host.py holds the two to each other bit for bit;
make_case()      _ref_ldpc.make_case with n = n_chain, decode_batch() the model over device-layout tensors; GRID / grid_case() / grid_expected()
                 and SPECIAL / special_case() / special_expected() are the cases of tests/test_ldpc_sc_gpu.py, built and decoded once.
"""
import functools

import numpy as np

import _ref_ldpc as B

F = np.float32
SIGMAS = (0.4, 0.55, 0.7)                                  # idle, decodable, undecodable (asserted in tests/test_ref_ldpc_sc_host.py)


def array_components(ms, nb, Z):
    """engine.sc_array_code's components[ms + 1, 1, nb]: shift (2^d (2c + 1)) mod Z in component d, column c."""
    d, c = np.arange(ms + 1)[:, None, None], np.arange(nb)[None, None, :]
    return ((2 ** d * (2 * c + 1)) % Z).astype(np.int32)


def holes_components(seed, ms, mb, nb, Z, keep):
    """Seeded random shifts; component d, row l keeps keep[d][l] non-zero blocks at seeded columns, the others are -1."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, Z, (ms + 1, mb, nb)).astype(np.int32)
    for d in range(ms + 1):
        for l in range(mb):
            s[d, l, rng.choice(nb, nb - keep[d][l], replace=False)] = -1
    return s


def coupled_shifts(comp, Lc):
    """shifts[(Lc + ms) mb, Lc nb] of the coupled matrix: block ((t, l), (i, c)) = comp[t - i][l][c] for 0 <= t - i <= ms."""
    comp = np.asarray(comp)
    ms, (mb, nb) = comp.shape[0] - 1, comp.shape[1:]
    s = np.full(((Lc + ms) * mb, Lc * nb), -1, np.int32)
    for i in range(Lc):
        for d in range(ms + 1):
            s[(i + d) * mb:(i + d + 1) * mb, i * nb:(i + 1) * nb] = comp[d]
    return s


def positions(ms, Lc, W):
    return max(1, Lc + ms - W + 1)


def decode(comp, Z, Lc, llr, bits, W, iters=10, alpha=0.75, T=None, stats=None):
    """-> (out[6] = iters, ok, post_err, pre_err, erased, iters_max; post[n_chain] float32; pos_err[Lc]; pos_iters[P]).
    stats: a dict whose "ties" gains the number of layer updates of a check in which two edges attained the minimum."""
    comp = np.asarray(comp)
    ms, (mb, nb) = comp.shape[0] - 1, comp.shape[1:]
    T = ms + 1 if T is None else T
    nbZ, ring, rows, P = nb * Z, W + ms, Lc + ms, positions(ms, Lc, W)
    llr = np.asarray(llr, F).reshape(Lc, nbZ)
    bits = np.asarray(bits).astype(bool).reshape(Lc, nbZ)
    a = F(alpha)
    ar = np.arange(Z)
    full = [[(d, c, int(comp[d, l, c])) for d in range(ms, -1, -1) for c in range(nb) if comp[d, l, c] >= 0] for l in range(mb)]
    Lr, Br = np.zeros(ring * nbZ, F), np.zeros(ring * nbZ, bool)                  # the ring of column blocks
    st = [[None] * mb for _ in range(W)]                                          # the ring of row blocks
    post, pos_err = np.zeros((Lc, nbZ), F), np.zeros(Lc, np.int64)

    def enter_col(i):
        k = (i % ring) * nbZ
        Lr[k:k + nbZ], Br[k:k + nbZ] = llr[i], bits[i]

    def leave_col(i):
        k = (i % ring) * nbZ
        post[i] = Lr[k:k + nbZ]
        pos_err[i] = int(((post[i] < 0) != Br[k:k + nbZ]).sum())

    def enter_row(t):
        for l in range(mb):                                                       # ring addresses of the edges row block (t, l) really has
            V = np.stack([((t - d) % ring) * nbZ + c * Z + (ar + s) % Z for d, c, s in full[l] if 0 <= t - d < Lc])
            st[t % W][l] = dict(V=V, sigma=np.bitwise_xor.reduce(Br[V], axis=0), m1=np.zeros(Z, F), m2=np.zeros(Z, F), idx=np.zeros(Z, np.int64),
                                sg=np.zeros(V.shape, bool))

    def passed(t_lo, t_hi):
        return all(not (np.bitwise_xor.reduce(Lr[s["V"]] < 0, axis=0) ^ s["sigma"]).any() for t in range(t_lo, t_hi) for s in st[t % W])

    def layer(s):
        V = s["V"]
        e = np.arange(V.shape[0])[:, None]
        mag = np.where(e == s["idx"], a * s["m2"], a * s["m1"]).astype(F)
        t = (Lr[V] - np.where(s["sg"], -mag, mag)).astype(F)
        A = np.abs(t)
        idx = np.argmin(A, axis=0)                                                # the first edge that attains the minimum
        m1 = A[idx, ar]
        A2 = A.copy()
        A2[idx, ar] = np.inf
        m2 = A2.min(axis=0)
        if stats is not None:
            stats["ties"] = stats.get("ties", 0) + int(((m1 == m2) & np.isfinite(m1)).sum())
        neg = t < 0
        S = np.bitwise_xor.reduce(neg, axis=0) ^ s["sigma"]
        nmag = np.where(e == idx, a * m2, a * m1).astype(F)
        nsg = S ^ neg
        Lr[V] = (t + np.where(nsg, -nmag, nmag)).astype(F)
        s.update(m1=m1, m2=m2, idx=idx, sg=nsg)

    pre_err, erased = int(((llr < 0) != bits).sum()), int((llr == 0).sum())
    for i in range(min(Lc, W)):
        enter_col(i)
    for t in range(min(W, rows)):
        enter_row(t)
    pos_iters, all_ok = np.zeros(P, np.int64), 1
    for p in range(P):
        t_hi = min(p + W, rows)
        t_test = min(p + T, rows) if p < P - 1 else t_hi
        n, ok = 0, passed(p, t_test)
        while not ok and n < iters:
            for t in range(p, t_hi):
                for s in st[t % W]:
                    layer(s)
            n += 1
            ok = passed(p, t_test)
        pos_iters[p] = n
        all_ok &= int(ok)
        if p == P - 1:
            break
        if p >= ms:
            leave_col(p - ms)
        if p + W < Lc:
            enter_col(p + W)
        if p + W < rows:
            enter_row(p + W)
    for i in range(max(P - 1 - ms, 0), Lc):
        leave_col(i)
    out = np.array([pos_iters.sum(), all_ok, pos_err.sum(), pre_err, erased, pos_iters.max()], np.int64)
    return out, post.reshape(-1), pos_err, pos_iters


def decode_scalar(comp, Z, Lc, llr, bits, W, iters=10, alpha=0.75, T=None):
    """The same figures from the dense coupled H, one check and one edge at a time, the full message of every edge kept as a float32 from the
    start of the call; a position is a range of rows of H and nothing else."""
    comp = np.asarray(comp)
    ms, (mb, nb) = comp.shape[0] - 1, comp.shape[1:]
    T = ms + 1 if T is None else T
    H = B.dense_H(coupled_shifts(comp, Lc), Z)
    rows = [np.nonzero(h)[0] for h in H]                       # ascending variable = ascending coupled block column: one edge per block
    L = [F(x) for x in np.asarray(llr, F)]
    b = [int(x) & 1 for x in bits]
    a = F(alpha)
    sigma = [sum(b[v] for v in r) & 1 for r in rows]
    pre_err = sum(int(x < 0) != y for x, y in zip(L, b))
    erased = sum(x == 0 for x in L)
    msg = [[F(0.0)] * len(r) for r in rows]
    mZ, nrow, P = mb * Z, Lc + ms, positions(ms, Lc, W)

    def test(lo, hi):
        return all((sum(int(L[v] < 0) for v in rows[k]) & 1) == sigma[k] for k in range(lo * mZ, hi * mZ))

    pos_iters, all_ok = [], 1
    for p in range(P):
        t_hi = min(p + W, nrow)
        t_test = min(p + T, nrow) if p < P - 1 else t_hi
        n, ok = 0, test(p, t_test)
        while not ok and n < iters:
            for k in range(p * mZ, t_hi * mZ):                 # rows in order = layers in order, and the checks of a layer in any order
                r = rows[k]
                t = [F(L[v] - msg[k][j]) for j, v in enumerate(r)]
                mags = [abs(x) for x in t]
                first = mags.index(min(mags))
                m1 = mags[first]
                m2 = min(x for j, x in enumerate(mags) if j != first)
                S = (sum(int(x < 0) for x in t) + sigma[k]) & 1
                for j, v in enumerate(r):
                    mag = F(a * (m2 if j == first else m1))
                    msg[k][j] = -mag if S ^ int(t[j] < 0) else mag
                    L[v] = F(t[j] + msg[k][j])
            n += 1
            ok = test(p, t_test)
        pos_iters.append(n)
        all_ok &= int(ok)
    post = np.array(L, F)
    wrong = ((post < 0) != np.array(b, bool)).reshape(Lc, nb * Z).sum(1)
    out = np.array([sum(pos_iters), all_ok, wrong.sum(), pre_err, erased, max(pos_iters)], np.int64)
    return out, post, wrong.astype(np.int64), np.array(pos_iters, np.int64)


def make_case(seed, n_chain, sigma, R, C, w, t0, erasures=4, plant=False):
    """_ref_ldpc.make_case for chains of n_chain bits; plant: also a +inf, a -inf and a -0.0 per run inside the chains (the erasures are +0.0)."""
    llr, bits = B.make_case(seed, n_chain, sigma, R, C, w, t0, erasures)
    if plant:
        rng = np.random.default_rng(seed + 77)
        for r in range(llr.shape[0]):
            g = rng.choice(C * n_chain, 3, replace=False)
            llr[r, g % w, t0 + g // w] = np.array([np.inf, -np.inf, -0.0], F)
    return llr, bits


def decode_batch(comp, Z, Lc, llr, bits, t0, C, W, iters=10, alpha=0.75, T=None, stats=None):
    """-> (out[R,C,6] int64, post[R,C,n_chain] float32, pos_err[R,C,Lc] int64, pos_iters[R,C,P] int64) of device-layout llr[R,w,N], bits[R,w,N]."""
    n = Lc * np.asarray(comp).shape[2] * Z
    lc, bc = B.codewords(llr, t0, C, n), B.codewords(bits, t0, C, n)
    res = [[decode(comp, Z, Lc, lc[r, c], bc[r, c], W, iters, alpha, T, stats) for c in range(C)] for r in range(llr.shape[0])]
    return tuple(np.array([[x[k] for x in row] for row in res]) for k in range(4))


# ------------------------------------------------------------------ the cases of tests/test_ldpc_sc_gpu.py, built and decoded once
A = array_components(2, 4, 31)
GRID = [(Lc, w, t0) for Lc, ws in ((12, (12, 8, 6)), (11, (12,))) for w in ws for t0 in (0, 7)]    # 11 x 124 = 1364 bits: chains start inside a symbol
GRID_W, GRID_ITERS, R_, C_ = 5, 10, 3, 2

# name: dict(comp, Z, Lc, W, iters, alpha, T, sigma, R, C, w, t0, plant, erasures)
_D = dict(comp=A, Z=31, Lc=12, W=5, iters=10, alpha=0.75, T=None, sigma=0.55, R=2, C=2, w=12, t0=5, plant=False, erasures=4)
SPECIAL = {
    "smallest-window": dict(_D, W=3),
    "one-position": dict(_D, W=14),
    "one-position-wide": dict(_D, Lc=6, W=11),
    "Lc-1": dict(_D, Lc=1, W=3, sigma=0.7),
    "Lc-ms": dict(_D, Lc=2, W=3, sigma=0.7),
    "test-1": dict(_D, T=1),
    "test-ms+1": dict(_D, T=3),
    "test-W": dict(_D, T=5),
    # ms = 1, mb = 2: the head rows (0, l) have 2 and 3 blocks, the tail rows (Lc, l) 3 and 2, the full rows 5
    "mb-2-holes": dict(_D, comp=holes_components(5, 1, 2, 6, 13, ((2, 3), (3, 2))), Z=13, Lc=9, W=4, sigma=0.8, w=8),
    "Z-64": dict(_D, comp=array_components(2, 4, 64), Z=64, Lc=6, W=4, R=1),
    "Z-65": dict(_D, comp=array_components(2, 4, 65), Z=65, Lc=6, W=4, R=1),
    "Z-80": dict(_D, comp=array_components(2, 4, 80), Z=80, Lc=6, W=4, R=1),
    "row-weight-32": dict(_D, comp=array_components(3, 8, 17), Z=17, Lc=7, W=5, sigma=0.4, R=1),
    "state-65520": dict(_D, comp=array_components(1, 6, 390), Z=390, Lc=4, W=3, sigma=0.6, R=1),
    # the probe's code on a chain of 36 360 bits: ms = 3, two waves per layer, 56 positions, the ring of 11 slots wraps five times
    "long-chain": dict(_D, comp=array_components(3, 6, 101), Z=101, Lc=60, W=8, sigma=0.53, R=1, C=1),
    "iters-1": dict(_D, iters=1, sigma=0.6),
    "iters-100": dict(_D, Lc=6, iters=100, sigma=0.62, R=1),
    "alpha-1": dict(_D, alpha=1.0),
    "alpha-0.5": dict(_D, alpha=0.5),
    "planted": dict(_D, plant=True, w=8, erasures=300),         # a tenth of the bits erased: checks with two zeros, a tie at the minimum
}

# Seeds for which the model shows what tests/test_ref_ldpc_sc_host.py asserts, as _ref_ldpc.RESEED
RESEED = {
    (12, 12, 0, 1): 100000, (12, 12, 7, 1): 60000, (12, 8, 7, 1): 20000, (12, 6, 0, 1): 20000, (12, 6, 7, 1): 10000,
    (12, 12, 0, 2): 10000, (12, 12, 7, 2): 30000, (12, 8, 0, 2): 30000, (12, 8, 7, 2): 10000, (12, 6, 0, 2): 10000, (12, 6, 7, 2): 10000,
}


def grid_seed(Lc, w, t0, level):
    return 5000 + 1000 * (Lc == 11) + 100 * level + 10 * (w // 2) + (t0 > 0) + RESEED.get((Lc, w, t0, level), 0)


@functools.lru_cache(maxsize=None)
def grid_case(Lc, w, t0, level):
    return make_case(grid_seed(Lc, w, t0, level), Lc * 124, SIGMAS[level], R_, C_, w, t0)


@functools.lru_cache(maxsize=None)
def grid_expected(Lc, w, t0, level):
    llr, bits = grid_case(Lc, w, t0, level)
    stats = {}
    return decode_batch(A, 31, Lc, llr, bits, t0, C_, GRID_W, GRID_ITERS, stats=stats) + (stats,)


@functools.lru_cache(maxsize=None)
def special_case(name):
    k = SPECIAL[name]
    n = k["Lc"] * k["comp"].shape[2] * k["Z"]
    return make_case(9000 + 10 * sorted(SPECIAL).index(name) + RESEED.get(name, 0), n, k["sigma"], k["R"], k["C"], k["w"], k["t0"], k["erasures"],
                     k["plant"])


@functools.lru_cache(maxsize=None)
def special_expected(name):
    k = SPECIAL[name]
    llr, bits = special_case(name)
    stats = {}
    return decode_batch(k["comp"], k["Z"], k["Lc"], llr, bits, k["t0"], k["C"], k["W"], k["iters"], k["alpha"], k["T"], stats) + (stats,)
