"""The integer model of vaeq_ldpc_sc_decode_q (include/vaeq.h): the sliding-window decoder of tests/_ref_ldpc_sc.py with the quantiser and the
integer layer update of tests/_ref_ldpc_q.py.  The header defines the call by reference to the two others, and so does this file: the window
schedule's helpers come from _ref_ldpc_sc, the quantiser, the limits and f from _ref_ldpc_q.

decode()         one chain, vectorised over the Z checks of a layer, the window kept as the kernel keeps it: a ring of W + ms column-block
                 slots for L (integers) and the TX bits, a ring of W row-block slots for the compressed state (m1, m2, idx, signs), idx an
                 edge's number in the FULL row as the header numbers it; `stats` (new_stats()) counts how often each rule binds;
decode_scalar()  an independent restatement: the rows of the dense coupled H as lists of variables, one explicit integer message per edge, all
                 L in one list, a quantiser of its own, no ring and no notion of entering or leaving -- tests/test_ref_ldpc_sc_q_host.py holds
                 the two to each other in every output;
decode_batch()   the model over device-layout tensors; GRID / grid_case() / grid_expected() and SPECIAL / special_case() / special_expected()
                 are the cases of tests/test_ldpc_sc_q_gpu.py, built and decoded once.
"""
import functools

import numpy as np

import _ref_ldpc as B
import _ref_ldpc_q as Q
import _ref_ldpc_sc as M

F = np.float32
DEFAULT = dict(bits=5, scale=1.0, app_bits=7, num=6, beta=0)                      # engine.resolve_quant(dict(bits=5))
IDENTITY = dict(bits=8, scale=1.0, app_bits=15, num=8, beta=0)                    # f(m) = m: the float decoder at alpha = 1 on small integers
# 5-bit decoding at scale 1 clips at +-15 nats.  The float cases' sigmas (0.4, 0.55, 0.7) need not suit it; these were chosen on the CPU so that
# tests/test_ref_ldpc_sc_q_host.py finds an idle chain, chains that decode after work and chains that fail; the seeds below (grid_seed,
# special_case) needed no re-drawing for that, so there is no RESEED table here.
SIGMAS = (0.25, 0.55, 0.75)
STATS = Q.STATS + ("ring_wraps", "head_rows", "tail_rows")


def new_stats():
    return dict.fromkeys(STATS, 0)


def decode(comp, Z, Lc, llr, bits, W, prm=DEFAULT, iters=10, T=None, stats=None):
    """-> (out[6] = iters, ok, post_err, pre_err, erased, iters_max; post[n_chain] int16; pos_err[Lc]; pos_iters[P]).
    stats: _ref_ldpc_q's counters, plus ring_wraps (a column block entered slot 0 again), head_rows / tail_rows (layer updates of a row block
    whose absent edges come first / last in the full row)."""
    comp = np.asarray(comp)
    ms, (mb, nb) = comp.shape[0] - 1, comp.shape[1:]
    T = ms + 1 if T is None else T
    nbZ, ring, rows, P = nb * Z, W + ms, Lc + ms, M.positions(ms, Lc, W)
    mmax, lmax = Q.limits(prm)
    raw = np.asarray(llr, F).reshape(Lc, nbZ)
    bits = np.asarray(bits).astype(bool).reshape(Lc, nbZ)
    quant = Q.quantise(raw, prm, stats if stats is not None else None)            # every bit of the chain passes the quantiser exactly once
    ar = np.arange(Z)
    full = [[(d, c, int(comp[d, l, c])) for d in range(ms, -1, -1) for c in range(nb) if comp[d, l, c] >= 0] for l in range(mb)]
    Lr, Br = np.zeros(ring * nbZ, np.int64), np.zeros(ring * nbZ, bool)           # the ring of column blocks
    st = [[None] * mb for _ in range(W)]                                          # the ring of row blocks
    post, pos_err = np.zeros((Lc, nbZ), np.int64), np.zeros(Lc, np.int64)

    def enter_col(i):
        k = (i % ring) * nbZ
        Lr[k:k + nbZ], Br[k:k + nbZ] = quant[i], bits[i]
        if stats is not None and i and i % ring == 0:
            stats["ring_wraps"] += 1

    def leave_col(i):
        k = (i % ring) * nbZ
        post[i] = Lr[k:k + nbZ]
        pos_err[i] = int(((post[i] < 0) != Br[k:k + nbZ]).sum())

    def enter_row(t):
        for l in range(mb):                                                       # the edges row block (t, l) really has, under their numbers in the full row
            E = np.array([e for e, (d, c, s) in enumerate(full[l]) if 0 <= t - d < Lc])
            V = np.stack([((t - d) % ring) * nbZ + c * Z + (ar + s) % Z for d, c, s in full[l] if 0 <= t - d < Lc])
            st[t % W][l] = dict(E=E, V=V, sigma=np.bitwise_xor.reduce(Br[V], axis=0), m1=np.zeros(Z, np.int64), m2=np.zeros(Z, np.int64),
                                idx=np.zeros(Z, np.int64), sg=np.zeros(V.shape, bool), head=E[0] > 0, tail=E[-1] < len(full[l]) - 1)

    def passed(t_lo, t_hi):
        return all(not (np.bitwise_xor.reduce(Lr[s["V"]] < 0, axis=0) ^ s["sigma"]).any() for t in range(t_lo, t_hi) for s in st[t % W])

    def layer(s):
        V, E = s["V"], s["E"][:, None]
        mag = Q._f(np.where(E == s["idx"], s["m2"], s["m1"]), prm)
        t = Lr[V] - np.where(s["sg"], -mag, mag)
        A = np.minimum(np.abs(t), mmax)
        k = np.argmin(A, axis=0)                                                  # the first edge that attains the minimum, after the clamp
        m1 = A[k, ar]
        A2 = A.copy()
        A2[k, ar] = 1 << 20
        m2 = A2.min(axis=0)
        idx = s["E"][k]
        neg = t < 0
        S = np.bitwise_xor.reduce(neg, axis=0) ^ s["sigma"]
        nmag = Q._f(np.where(E == idx, m2, m1), prm)
        nsg = S ^ neg
        u = t + np.where(nsg, -nmag, nmag)
        Lr[V] = np.clip(u, -lmax, lmax)
        if stats is not None:
            stats["message_clamp"] += int((np.abs(t) > mmax).sum())
            stats["app_clamp"] += int((np.abs(u) > lmax).sum())
            stats["f_zero"] += int(((Q._f(m1, prm) == 0) & (m1 > 0)).sum() + ((Q._f(m2, prm) == 0) & (m2 > 0)).sum())
            stats["tie_not_first"] += int((((A == m1).sum(axis=0) > 1) & (k > 0)).sum())
            stats["t_zero"] += int((t == 0).sum())
            stats["head_rows"] += int(s["head"])
            stats["tail_rows"] += int(s["tail"])
        s.update(m1=m1, m2=m2, idx=idx, sg=nsg)

    with np.errstate(invalid="ignore"):
        pre_err = int(((raw < 0) != bits).sum())                                  # of the raw input; a NaN is bit 0
    erased = int((quant == 0).sum())
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
    return out, post.reshape(-1).astype(np.int16), pos_err, pos_iters


def decode_scalar(comp, Z, Lc, llr, bits, W, prm=DEFAULT, iters=10, T=None):
    """The same figures one check and one edge at a time: the rows of the dense coupled H as lists of their variables (ascending variable =
    ascending coupled block column: one edge per block), the full message of every edge kept as a Python int from the start of the call; a
    position is a range of rows of H and nothing else.  (H itself is not materialised: a chain of 36 360 bits has 2 x 10^8 cells.)"""
    comp = np.asarray(comp)
    ms, (mb, nb) = comp.shape[0] - 1, comp.shape[1:]
    T = ms + 1 if T is None else T
    sh = M.coupled_shifts(comp, Lc)
    rows = [sorted(c * Z + (i + int(sh[r, c])) % Z for c in np.nonzero(sh[r] >= 0)[0]) for r in range(sh.shape[0]) for i in range(Z)]
    cmax = mmax = 2 ** (prm["bits"] - 1) - 1
    lmax = 2 ** (prm["app_bits"] - 1) - 1
    num, beta, scale = int(prm["num"]), int(prm["beta"]), F(prm["scale"])
    b = [int(x) & 1 for x in bits]
    L, pre_err = [], 0
    for x, y in zip(np.asarray(llr, F), b):
        pre_err += int(bool(x < 0)) != y
        with np.errstate(all="ignore"):
            v = F(x * scale)
        if v != v:
            v = F(0.0)
        v = F(min(max(v, F(-cmax)), F(cmax)))
        lo = int(np.floor(v))
        d = float(v) - lo                                      # exact: |v| <= 127 in float32
        L.append(lo if d < 0.5 else lo + 1 if d > 0.5 else lo + (lo & 1))   # a tie goes to the even neighbour
    erased = sum(x == 0 for x in L)
    sigma = [sum(b[v] for v in r) & 1 for r in rows]
    msg = [[0] * len(r) for r in rows]
    f = [max(((num * a + 4) >> 3) - beta, 0) for a in range(mmax + 1)]
    mZ, nrow, P = mb * Z, Lc + ms, M.positions(ms, Lc, W)

    def test(lo, hi):
        return all((sum(L[v] < 0 for v in rows[k]) & 1) == sigma[k] for k in range(lo * mZ, hi * mZ))

    pos_iters, all_ok = [], 1
    for p in range(P):
        t_hi = min(p + W, nrow)
        t_test = min(p + T, nrow) if p < P - 1 else t_hi
        n, ok = 0, test(p, t_test)
        while not ok and n < iters:
            for k in range(p * mZ, t_hi * mZ):                 # rows in order = layers in order, and the checks of a layer in any order
                r, mk = rows[k], msg[k]
                t = [L[v] - m for v, m in zip(r, mk)]
                mags = [min(abs(x), mmax) for x in t]
                m1 = min(mags)
                first = mags.index(m1)
                m2 = min(mags[:first] + mags[first + 1:])
                S = sigma[k]
                for x in t:
                    S ^= x < 0
                for j, v in enumerate(r):
                    mag = f[m2 if j == first else m1]
                    mk[j] = -mag if S ^ (t[j] < 0) else mag
                    L[v] = min(max(t[j] + mk[j], -lmax), lmax)
            n += 1
            ok = test(p, t_test)
        pos_iters.append(n)
        all_ok &= int(ok)
    post = np.array(L, np.int64)
    wrong = ((post < 0) != np.array(b, bool)).reshape(Lc, nb * Z).sum(1)
    out = np.array([sum(pos_iters), all_ok, wrong.sum(), pre_err, erased, max(pos_iters)], np.int64)
    return out, post.astype(np.int16), wrong.astype(np.int64), np.array(pos_iters, np.int64)


def decode_batch(comp, Z, Lc, llr, bits, t0, C, W, prm=DEFAULT, iters=10, T=None, stats=None):
    """-> (out[R,C,6] int64, post[R,C,n_chain] int16, pos_err[R,C,Lc] int64, pos_iters[R,C,P] int64) of device-layout llr[R,w,N], bits[R,w,N]."""
    n = Lc * np.asarray(comp).shape[2] * Z
    lc, bc = B.codewords(llr, t0, C, n), B.codewords(bits, t0, C, n)
    res = [[decode(comp, Z, Lc, lc[r, c], bc[r, c], W, prm, iters, T, stats) for c in range(C)] for r in range(llr.shape[0])]
    return tuple(np.array([[x[k] for x in row] for row in res]) for k in range(4))


def small_integer_case(seed, n_chain, R, C, w, t0, sigma=0.55, gain=3, amp=6):
    """LLRs that are small integers: rint(gain y) clipped to +-amp of y = (1 - 2 b) + sigma noise, a zero always +0.0.  Float32 min-sum at
    alpha = 1 stays on integers with such an input, and IDENTITY quantises nothing away."""
    rng = np.random.default_rng(seed)
    N = t0 + -(-C * n_chain // w) + 3
    bits = rng.integers(0, 2, (R, w, N)).astype(np.int8)
    y = (1.0 - 2.0 * bits) + sigma * rng.standard_normal((R, w, N))
    return (np.clip(np.rint(gain * y), -amp, amp) + 0.0).astype(F), bits          # (+ 0.0: no -0.0 among the erasures)


# ------------------------------------------------------------------ the cases of tests/test_ldpc_sc_q_gpu.py, built and decoded once
A = M.A
GRID, GRID_W, GRID_ITERS, R_, C_ = M.GRID, M.GRID_W, M.GRID_ITERS, M.R_, M.C_

# The float window tests' corners (alpha has no meaning here) at the 5-bit defaults, then one corner per rule of the quantiser.
# name: dict(comp, Z, Lc, W, iters, T, sigma, R, C, w, t0, plant, erasures, prm, q_plant): plant = _ref_ldpc_sc's +-inf and -0.0, q_plant =
# _ref_ldpc_q's +-0.5, +-1.5, +-2.5 over the scale, a +inf and a NaN.
_D = dict(M._D, prm=DEFAULT, q_plant=False)
SPECIAL = {name: dict(k, prm=DEFAULT, q_plant=False) for name, k in M.SPECIAL.items() if not name.startswith("alpha-")}
SPECIAL.update({
    "bits-2": dict(_D, prm=dict(bits=2, scale=0.125, app_bits=2, num=6, beta=0)),
    "bits-8": dict(_D, prm=dict(bits=8, scale=8.0, app_bits=15, num=6, beta=0)),
    "offset-min-sum": dict(_D, prm=dict(DEFAULT, num=8, beta=1)),
    "scale-1e-30": dict(_D, prm=dict(DEFAULT, scale=1e-30)),                    # everything is erased
    "scale-1e30": dict(_D, prm=dict(DEFAULT, scale=1e30)),                      # everything is clipped, the erasures stay
    "planted-q": dict(_D, q_plant=True, w=8, prm=dict(DEFAULT, scale=0.5)),
    # ms = 1, nb = 9, W = 3: 132 Z bytes; Z = 496 is 65 472, Z = 497 is 65 604
    "state-65472": dict(_D, comp=M.array_components(1, 9, 496), Z=496, Lc=4, W=3, sigma=0.6, R=1),
    "app-narrow": dict(_D, prm=dict(DEFAULT, app_bits=5)),                      # Lmax = Mmax: the a-posteriori clamp binds
})
for _k in SPECIAL.values():
    _k.pop("alpha", None)

def grid_seed(Lc, w, t0, level):
    return 15000 + 1000 * (Lc == 11) + 100 * level + 10 * (w // 2) + (t0 > 0)


@functools.lru_cache(maxsize=None)
def grid_case(Lc, w, t0, level):
    return M.make_case(grid_seed(Lc, w, t0, level), Lc * 124, SIGMAS[level], R_, C_, w, t0)


@functools.lru_cache(maxsize=None)
def grid_expected(Lc, w, t0, level):
    llr, bits = grid_case(Lc, w, t0, level)
    stats = new_stats()
    return decode_batch(A, 31, Lc, llr, bits, t0, C_, GRID_W, DEFAULT, GRID_ITERS, stats=stats) + (stats,)


@functools.lru_cache(maxsize=None)
def special_case(name):
    k = SPECIAL[name]
    n = k["Lc"] * k["comp"].shape[2] * k["Z"]
    seed = 19000 + 10 * sorted(SPECIAL).index(name)
    llr, bits = M.make_case(seed, n, k["sigma"], k["R"], k["C"], k["w"], k["t0"], k["erasures"], k["plant"])
    if k["q_plant"]:
        w, t0 = k["w"], k["t0"]
        llr = Q._plant(llr.copy(), seed + 7777, k["prm"]["scale"], k["R"], lambda g: (g % w, t0 + g // w), k["C"] * n, True)
    return llr, bits


@functools.lru_cache(maxsize=None)
def special_expected(name):
    k = SPECIAL[name]
    llr, bits = special_case(name)
    stats = new_stats()
    return decode_batch(k["comp"], k["Z"], k["Lc"], llr, bits, k["t0"], k["C"], k["W"], k["prm"], k["iters"], k["T"], stats) + (stats,)


@functools.lru_cache(maxsize=None)
def identity_case():
    """The input of the device-against-device identity with the float window decoder at alpha = 1 (Lc = 12, w = 8, t0 = 7, R_ x C_ chains)."""
    return small_integer_case(17000, 12 * 124, R_, C_, 8, 7)
