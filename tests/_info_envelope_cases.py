"""The cases of tests/test_info_envelope_gpu.py, tests/test_awgn_info_envelope_gpu.py and tests/test_ref_info_envelope_host.py: what the eight
information-rate and LLR entry points (vaeq_dp_epilogue_info / _llr, vaeq_awgn_info / _llr, vaeq_cma_epilogue_info / _llr, vaeq_awgn_track_info /
_llr, include/vaeq.h) accept and the cases of their feature commits leave out.  No new model: every run is made by a generator of
tests/_ref_info.py, _ref_awgn_info.py, _ref_cma_info.py or _ref_awgn_baseline_info.py and evaluated by that file's float64 model, once per process
(dp(), cma(), awgn(), track(): lru_cache, arrays frozen).

One entry of DP / CMA / AWGN / TRACK is one kernel launch of R <= 8 runs that share what a launch shares (N, n_lev, batch_len, edge, layout);
`kept` is the number of symbols every run keeps (DP and CMA: of polarisation 0 and 1), written here and asserted by the host test, so that no
window is empty, or full, by accident.  A run that misses a floor of its pair advances its seed; no floor is lowered and no case is dropped.

DP, by the items of the issue (the name's prefix):
  shift-    every shift[0] in -10 .. 10 with an unequal shift[1] at N = 300, batch_len 0, seven per launch;
  N         N in {43 .. 47, 255, 256, 257, 511, 512, 513} without a cut (the LLR grid's block edge, the info kernel's second and third strided
            round), and N = 20011 (a fixed-order float sum over 78 terms per thread);
  B         (batch_len, N) with shift[0] in {-10, -9, 0, 5, 10}: batch_len < 20 (a negative slice end), >= 256 (KeepWalk's dq = 0), == 256
            (dr = 0), == N; B1-N64 keeps something at shift[0] = -10 alone; B20-N60 has the run with shift (0, -7) that keeps ONE symbol, and
            its windows at shift[0] in {5, 10} are empty: kept and empty runs in one launch;
  clamp     runs built at shifts of +-10 whose `wild` shifts (+-11, +-1000, INT32_MIN, INT32_MAX) the kernels clamp to those;
  stride    three runs that differ in shift, r, hyp and var at N = 43, n_lev = 2: the base of the R = 16385 launch.
CMA: N in {43 .. 46, 257}; all 16 combinations of shift_c and shift_q in the four extremes with all four (r_c, r_q) at N = 43; scale_edges on
and off (a wrapped sample outside W_c stays unscaled).  AWGN: the short rows, every shift in -10 .. 12 over N in {255, 256, 257, 513}, N = 20011,
and `wild` shifts whose window is empty.  TRACK: (Nd, edge, shift) x layout x (Nz - Nd), and the int32 extremes of shift and edge.
PLANTED_DP / PLANTED_AWGN: the hand-made q-mode edges (ties of posteriors and of hypotheses, TX samples off the grid, subnormal posteriors, a
pmf with zero entries), built by planted_dp() / planted_awgn().
"""
import functools

import numpy as np

import _ref_awgn_baseline_info as T
import _ref_awgn_info as A
import _ref_cma_info as C
import _ref_epilogue as E
import _ref_info as I

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
EXTREMES = [(10, -10), (-10, 10), (10, 10), (-10, -10)]
WILD = (11, -11, 1000, -1000, INT32_MIN, INT32_MAX)


def clamp(s):
    return max(-10, min(10, int(s)))


class _Hyps:
    """The planted hypothesis of the next run at n_lev = n: each n_lev walks through all of them."""

    def __init__(self, nh):
        self.nh, self.c = nh, {2: 0, 4: 0, 8: 0}

    def __call__(self, n):
        h = self.c[n] % self.nh
        self.c[n] += 1
        return h


def _freeze(x):
    for v in x.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x


def _nu(i):
    return (0.0, I.NU_SHAPED)[i % 2]


# ------------------------------------------------------------------ the DP pair
def _dp_launches():
    hyp, L, seed = _Hyps(8), {}, [30000]

    def run(N, n, shift, r, B, i, **kw):
        seed[0] += 10
        return dict(seed=seed[0], N=N, n=n, shift=tuple(shift), r=r, hyp=hyp(n), batch_len=B, nu=_nu(i + n),
                    var=(0.003 + 0.001 * (i % 3), 0.006 - 0.001 * (i % 2)), n_err=(1 + i % 3, 3 - i % 3), **kw)

    for j, n in enumerate((2, 4, 8)):
        L[f"shift-n{n}"] = [run(300, n, (s0, E._other(s0, i)), (i + j) % 2, None, i) for i, s0 in enumerate(range(-10 + j, 11, 3))]
    for j, N in enumerate((43, 44, 45, 46, 47, 255, 256, 257, 511, 512, 513)):
        L[f"N{N}"] = [run(N, (2, 4, 8)[j % 3], s, (i + j) % 2, None, i) for i, s in enumerate([(10, -10), (-10, 10), (3, -7), (0, 0)])]
    L["N20011"] = [run(20011, 8, (10, -3), 0, None, 0), run(20011, 8, (-4, -10), 1, None, 1)]
    for j, (B, N) in enumerate([(1, 64), (10, 100), (14, 140), (19, 190), (20, 60), (255, 510), (256, 512), (257, 771), (300, 600), (1000, 2000),
                                (100, 100), (257, 257)]):
        n = 2 if (B, N) == (20, 60) else (8, 4, 2)[j % 3]                      # (one kept symbol ties two hypotheses at n_lev = 2 whatever it is)
        runs = [run(N, n, (s0, E._other(s0, i + j)), (i + j) % 2, B, i) for i, s0 in enumerate((-10, -9, 0, 5, 10))]
        if (B, N) == (20, 60):
            runs.append(run(N, n, (0, -7), 0, B, 5))
        L[f"B{B}-N{N}"] = runs
    for B, n in ((None, 4), (100, 8)):
        L[f"clamp-B{B or 0}"] = [run(300, n, (clamp(w), clamp(WILD[5 - i])), i % 2, B, i, wild=(w, WILD[5 - i])) for i, w in enumerate(WILD)]
    L["stride"] = [dict(seed=39000 + i, N=43, n=2, shift=s, r=r, hyp=h, batch_len=None, nu=_nu(i), var=v, n_err=(1, 2))
                   for i, (s, r, h, v) in enumerate([((10, -10), 0, 5, (0.003, 0.006)), ((-3, 7), 1, 2, (0.005, 0.004)), ((0, 4), 0, 7, (0.004, 0.003))])]
    return L


DP = _dp_launches()
# kept symbols of polarisation 0 (= of polarisation 1: the window is the run's), per run
DP_KEPT = {
    "shift-n2": [268, 271, 274, 270, 270, 270, 270], "shift-n4": [269, 272, 274, 269, 271, 269, 269], "shift-n8": [270, 273, 273, 268, 272, 268, 268],
    "N43": [11, 11, 14, 21], "N44": [12, 12, 15, 22], "N45": [13, 13, 16, 23], "N46": [14, 14, 17, 24], "N47": [15, 15, 18, 25],
    "N255": [223, 223, 226, 233], "N256": [224, 224, 227, 234], "N257": [225, 225, 228, 235], "N511": [479, 479, 482, 489],
    "N512": [480, 480, 483, 490], "N513": [481, 481, 484, 491], "N20011": [19979, 19979],
    # batch_len B, shift[0] = s: Lk = B - s - 10 symbols of each minibatch (B + that where it is negative, none below 0), K = (N / B) Lk of the frame,
    # K - 22 - max|shift| kept: B1-N64 keeps 64 - 32 at s = -10 and has Lk = 0 otherwise; B20-N60 at s in {5, 10} has K = 15 and 0
    "B1-N64": [32, 0, 0, 0, 0], "B10-N100": [68, 59, 0, 23, 0], "B14-N140": [108, 99, 8, 100, 48], "B19-N190": [158, 149, 65, 8, 148],
    "B20-N60": [28, 26, 3, 0, 0, 1], "B255-N510": [478, 477, 461, 451, 438], "B256-N512": [480, 479, 461, 455, 440],
    "B257-N771": [739, 737, 709, 696, 679], "B300-N600": [568, 567, 555, 538, 528], "B1000-N2000": [1968, 1967, 1953, 1939, 1928],
    "B100-N100": [68, 68, 61, 56, 48], "B257-N257": [225, 225, 216, 215, 205],
    "clamp-B0": [268, 268, 268, 268, 268, 268], "clamp-B100": [208, 268, 208, 268, 268, 208], "stride": [11, 14, 17],
}
CMA_KEPT = {"N43": [19, 18, 21, 11], "N44": [20, 19, 22, 12], "N45": [21, 20, 23, 13], "N46": [22, 21, 24, 14], "N257": [233, 232, 235, 225],
            "extremes0-n8": [11] * 8, "extremes1-n2": [11] * 8, "extremes-N257-n4": [225] * 6}
AWGN_KEPT = {"N255": [243, 239, 235, 231, 227, 223], "N256": [243, 239, 235, 231, 227, 223], "N257": [243, 239, 235, 231, 227, 223],
             "N513": [498, 494, 490, 486, 482], "N20011": [19977, 19999], "wild": [0, 0, 0, 0, 0, 0, 35, 48]}      # N - 22 - shift; the short rows: AWGN_SHORT
TRACK_WILD_KEPT = {"wild-shift": [0, 0, 0, 0, 34], "wild-edge": [0, 0, 0]}


def dp_floors_ok(mq, my):
    if mq["kept"][0] == 0:
        return True
    return mq["min_post"] >= I.MIN_POST_FLOOR and mq["qgap"] >= E.QGAP_FLOOR and my["qgap"] >= E.QGAP_FLOOR


def dp_models(x):
    return (I.info_q(x["q"], x["tx"], x["P"], x["shift"], x["r"], x["batch_len"]),
            I.info_y(x["y"], x["tx"], x["P"], x["amp"], x["nu_sc"], x["var"], x["shift"], x["r"], x["batch_len"]))


def dp_run(spec):
    """_ref_info.make_run at the first seed from spec's on whose models meet the floors -> (x, mq, my)."""
    kw = {k: v for k, v in spec.items() if k != "wild"}
    for seed in range(spec["seed"], spec["seed"] + 200):
        x = I.make_run(**dict(kw, seed=seed))
        mq, my = dp_models(x)
        if dp_floors_ok(mq, my):
            if "wild" in spec:
                x["wild"] = np.asarray(spec["wild"], np.int64)
            return _freeze(x), mq, my
    raise RuntimeError(f"no seed meets the floors for {spec}")


@functools.lru_cache(maxsize=None)
def dp(name):
    """-> (per-run inputs, per-run q-mode model results, per-run y-mode model results)."""
    return tuple(map(list, zip(*[dp_run(s) for s in DP[name]])))


# ------------------------------------------------------------------ the CMA pair
def _cma_launches():
    hyp, L, seed = _Hyps(8), {}, [40000]

    def run(N, n, sc, sq, rc, rq, i, edges=None):
        seed[0] += 10
        return dict(seed=seed[0], N=N, n=n, shift_c=sc, r_c=rc, shift_q=sq, r_q=rq, hyp=hyp(n), s=C.SCALES[i % 3], nu=_nu(i + n),
                    var=(0.003 + 0.001 * (i % 3), 0.006 - 0.001 * (i % 2)), n_err=(1 + i % 2, 2 - i % 2), scale_edges=bool(i % 2) if edges is None else edges)

    for j, N in enumerate((43, 44, 45, 46, 257)):
        L[f"N{N}"] = [run(N, (4, 2, 8)[j % 3], EXTREMES[(i + j) % 4], [(2, -1), (-3, 3), (0, 0), (10, -4)][i], i % 2, (i >> 1) % 2, i) for i in range(4)]
    combos = [(sc, sq) for sc in EXTREMES for sq in EXTREMES]
    for half, n in ((0, 8), (1, 2)):
        L[f"extremes{half}-n{n}"] = [run(43, n, sc, sq, (i + half) % 2, ((i >> 1) + half) % 2, i, None if n == 2 else False) for i, (sc, sq) in enumerate(combos[8 * half:8 * half + 8])]
    L["extremes-N257-n4"] = [run(257, 4, sc, sq, i % 2, (i >> 1) % 2, i) for i, (sc, sq) in enumerate(combos[5::2])]
    return L


CMA = _cma_launches()


@functools.lru_cache(maxsize=None)
def cma(name):
    """-> (per-run inputs, per-run model results)."""
    xs, ms = [], []
    for spec in CMA[name]:
        x, m = C.build_run(**spec)
        xs.append(_freeze(x))
        ms.append(m)
    return xs, ms


# ------------------------------------------------------------------ the AWGN pair
AWGN_SHORT = [(1, 0, 0), (12, -10, 0), (13, -10, 1), (14, -10, 2), (22, -10, 10), (23, 0, 1), (34, 11, 1), (35, 12, 1)]     # N, shift, kept


def _awgn_launches():
    hyp, L, seed = _Hyps(4), {}, [50000]

    def run(N, n, shift, i, **kw):
        seed[0] += 300
        var = A.VARS[i % 3]
        return dict(seed=seed[0], N=N, n=n, shift=shift, hyp=hyp(n), nu=_nu(i + n), var=var, n_err=i % 3, **kw)

    for j, (N, sh, _) in enumerate(AWGN_SHORT):
        n = 2 if N == 1 else (2, 4, 8)[j % 3]                                    # (no seed meets the floors for N = 1 at n_lev = 8)
        L[f"N{N}-s{sh}"] = [run(N, n, sh, i) for i in range(3)]
    shifts = list(range(-10, 13))
    for j, N in enumerate((255, 256, 257, 513)):
        L[f"N{N}"] = [run(N, (8, 4, 2)[j % 3], sh, i) for i, sh in enumerate(shifts[j::4])]
    L["N20011"] = [run(20011, 8, 12, 0), run(20011, 8, -10, 1)]
    L["wild"] = [run(60, 4, 0, i, wild=w) for i, w in enumerate((-11, -1000, INT32_MIN, INT32_MAX, 60, 38))] + [run(60, 4, 3, 6), run(60, 4, -10, 7)]
    return L


AWGN = _awgn_launches()


@functools.lru_cache(maxsize=None)
def awgn(name):
    """-> (per-run inputs, per-run q-mode model results, per-run y-mode model results); a `wild` run is built at shift 0 and carries the shift the
    kernels get (its window is empty) in x["shift"]."""
    xs, mq, my = [], [], []
    for spec in AWGN[name]:
        x, a, b = A.conditioned_run({k: v for k, v in spec.items() if k != "wild"})
        if "wild" in spec:
            x["shift"] = int(spec["wild"])
            a, b = A.models(x)
        xs.append(_freeze(x))
        mq.append(a)
        my.append(b)
    return xs, mq, my


# ------------------------------------------------------------------ the track pair
TRACK_GEOM = [(30, 0, 5, 25), (30, 0, 0, 0), (30, 1, 0, 28), (30, 1, 3, 25), (64, 20, 11, 13), (255, 11, -12, 0), (256, 11, 11, 223), (257, 31, -12, 207),
              (513, 100, 7, 306), (300, 149, 0, 2), (300, 150, 0, 0)]            # Nd, edge, shift, kept


def _track_launches():
    hyp, L, seed = _Hyps(4), {}, [60000]

    def run(Nd, dz, e, il, n, shift, i, **kw):
        seed[0] += 5000
        var = A.VARS[i % 3]
        return dict(seed=seed[0], Nd=Nd, dz=dz, e=e, n=n, shift=shift, hyp=hyp(n), nu=_nu(i + n), var=var, n_err=T.feasible_errors(n, var, 1 + i % 2),
                    gain=T.GAINS[i % 3], interleaved=bool(il), **kw)

    a = 0
    for Nd, e, sh, _ in TRACK_GEOM:
        for dz in (0, 1):
            for il in (0, 1):
                n = (2, 4, 8)[a % 3]
                L[f"Nd{Nd}-e{e}-s{sh}-dz{dz}-il{il}"] = [run(Nd, dz, e, il, n, sh, a + i) for i in range(2)]
                a += 1
    for il in (0, 1):
        L[f"wild-shift-il{il}"] = [run(60, il, 11, il, 8, 0, i, wild_shift=w) for i, w in enumerate((INT32_MIN, INT32_MAX, 38, -11))] + [run(60, il, 11, il, 8, 4, 5)]
        L[f"wild-edge-il{il}"] = [run(60, 1 - il, 11, il, 4, s, i, wild_edge=INT32_MAX) for i, s in enumerate((0, -12, 11))]
    return L


TRACK = _track_launches()


@functools.lru_cache(maxsize=None)
def track(name):
    """-> (per-run inputs, per-run model results); a `wild_shift` / `wild_edge` run is built at its spec's shift and edge and carries what the
    kernels get (its window is empty) in x["shift"] / x["edge"]."""
    xs, ms = [], []
    for spec in TRACK[name]:
        x, m = T.conditioned_run({k: v for k, v in spec.items() if not k.startswith("wild")})
        if "wild_shift" in spec:
            x["shift"] = int(spec["wild_shift"])
        if "wild_edge" in spec:
            x["edge"] = int(spec["wild_edge"])
        if "wild_shift" in spec or "wild_edge" in spec:
            m = T.model(x)
        xs.append(_freeze(x))
        ms.append(m)
    return xs, ms


# ------------------------------------------------------------------ planted edges (q-mode: the counts are exact whatever the posterior gap)
def _tie_dp(h1, h2, n, seed0):
    """A DP run (shift 0, r 0) in which hypotheses h1 < h2 tie for the fewest symbol errors in BOTH polarisations -> (x, mq)."""
    N = 60
    idx = E.kept_indices(N, (0, 0), None)
    for seed in range(seed0, seed0 + 400):
        kw = dict(seed=seed, N=N, n=n, shift=(0, 0), r=0, batch_len=None, nu=0.0, var=(0.004, 0.004), n_err=(0, 0))
        x1, x2 = I.make_run(**dict(kw, hyp=h1)), I.make_run(**dict(kw, hyp=h2))
        q = x1["q"].copy()
        ok = True
        for p in range(2):
            found = False
            for cut in range(len(idx) // 2 - 6, len(idx) // 2 + 7):
                q[p] = x1["q"][p]
                q[p][:, idx[cut]:] = x2["q"][p][:, idx[cut]:]
                c = I.info_q(q, x1["tx"], x1["P"], (0, 0), 0)["cnt"][:, p]
                if c[h1] == c[h2] == c.min() and (c == c.min()).sum() == 2:
                    found = True
                    break
            ok = ok and found
        if ok:
            x = dict(x1, q=q, hyp=h1)
            return _freeze(x), I.info_q(q, x["tx"], x["P"], (0, 0), 0)
    raise RuntimeError(f"no tie of hypotheses {h1} and {h2} found")


def _tie_awgn(h1, h2, n, seed0):
    N = 60
    ri, ti = A.window(N, 0)
    for seed in range(seed0, seed0 + 400):
        kw = dict(seed=seed, N=N, n=n, shift=0, nu=0.0, var=0.004, n_err=0)
        x1, x2 = A.make_run(**dict(kw, hyp=h1)), A.make_run(**dict(kw, hyp=h2))
        for cut in range(len(ri) // 2 - 6, len(ri) // 2 + 7):
            q = x1["q"].copy()
            q[:, ri[cut]:] = x2["q"][:, ri[cut]:]
            m = A.info_q(q, x1["tx"], x1["P"], 0)
            c = m["cnt"]
            if c[h1] == c[h2] == c.min() and (c == c.min()).sum() == 2:
                return _freeze(dict(x1, q=q, hyp=h1)), m
    raise RuntimeError(f"no tie of hypotheses {h1} and {h2} found")


def _gray_set(n, k, v):
    g = I.gray(np.arange(n))
    return np.flatnonzero(((g >> k) & 1) == v)


F16 = np.float16
HALF_ULP_4 = (F16(0.66650390625), F16(0.6669921875))             # the float16 neighbours of 2 / 3: 1.5 t + 1.5 is 2.49976 (level 2) and 2.50049 (level 3)
HALF_ULP_8 = (F16(0.28564453125), F16(0.2858886718750))          # ... of 2 / 7: 3.5 t + 3.5 is 4.49976 (level 4) and 4.50061 (level 5)


def off_grid_tx(n):
    """TX samples off the level grid -> (values float16, the levels clamp(rint((n-1)/2 t + (n-1)/2), 0, n-1) with ties to even, worked out by hand)."""
    if n == 2:
        return np.array([0.0, -0.0, 2.0 ** -10, -2.0 ** -10, 1.5, -1.5, 3.0, 60000.0], F16), np.array([0, 0, 1, 0, 1, 0, 1, 1])
    if n == 4:
        return np.array([HALF_ULP_4[0], HALF_ULP_4[1], -HALF_ULP_4[0], -HALF_ULP_4[1], 1.0 / 3, -1.0, 1.5, -1.5], F16), np.array([2, 3, 1, 0, 2, 0, 3, 0])
    return np.array([HALF_ULP_8[0], HALF_ULP_8[1], -HALF_ULP_8[0], -HALF_ULP_8[1], 1.0, 1.5, -1.5, -60000.0], F16), np.array([4, 5, 3, 2, 7, 7, 0, 0])


PLANTED_POS = (13, 17, 22, 30, 31, 40, 44, 47)                  # kept TX indices of the planted runs (N = 60, shift 0: the window is [11, 49))
SUBNORMAL = np.float32(1e-40)


def _plant(pair, kind, n, seed):
    """One planted q-mode run of `pair` ("dp" / "awgn") at N = 60, shift 0 (DP: r = 0, no cut): the generator's run with PLANTED_POS changed."""
    N, S = 60, n - 1
    dp_ = pair == "dp"
    P = None
    if kind == "pmf-zeros":
        P = np.zeros(n)                                                       # (n_lev = 2: the one-level pmf is the only one with a zero)
        P[[0, n - 1] if n > 2 else [1]] = 0.5 if n > 2 else 1.0
    elif kind == "pmf-one-level":
        P = np.zeros(n)
        P[n // 2] = 1.0
    if dp_:
        x = dict(I.make_run(seed=seed, N=N, n=n, shift=(0, 0), r=0, hyp=0, batch_len=None, nu=0.0, var=(0.004, 0.004), n_err=(1, 2), P=P))
        q, tx = x["q"].copy().reshape(2, 2, n, N), x["tx"].copy()
        rows = [(p, c) for p in range(2) for c in range(2)]
    else:
        x = dict(A.make_run(seed=seed, N=N, n=n, shift=0, hyp=0, nu=0.0, var=0.004, n_err=1, P=P))
        q, tx = x["q"].copy().reshape(1, 2, n, N), x["tx"].copy()[None]
        rows = [(0, c) for c in range(2)]
    lev = I.tx_levels(tx, n)
    for k, pos in enumerate(PLANTED_POS):
        p, c = rows[k % len(rows)]
        t = int(lev[p, c, pos])
        if kind == "posterior-tie":                                           # two equal top posteriors: the first maximum decides
            lo, hi = (t - 1, t) if (k % 2 == 0 and t > 0) or t == S else (t, t + 1)
            q[p, c, :, pos] = np.float32(0.2 / max(n - 2, 1)) if n > 2 else 0.0
            q[p, c, lo, pos] = q[p, c, hi, pos] = np.float32(0.4 if n > 2 else 0.5)
        elif kind == "off-grid":
            tx[p, c, pos] = off_grid_tx(n)[0][k]
        elif kind == "subnormal":
            # 0.8 at S - t (the level whose label differs from t's in the top bit alone), the rest spread: one level dominates, so the signs of the
            # LLRs still are the bits of the decision
            q[p, c, :, pos] = np.float32(0.2 / max(n - 1, 1))
            q[p, c, S - t, pos] = np.float32(0.8)
            if k % 2 == 0 or n == 2:                                          # the transmitted level's posterior is subnormal
                q[p, c, t, pos] = SUBNORMAL
            else:                                                             # a whole bit-wise set (the transmitted top bit's) sums to a subnormal
                kb = int(np.log2(n)) - 1
                q[p, c, _gray_set(n, kb, (int(I.gray(t)) >> kb) & 1), pos] = SUBNORMAL
    x["q"] = q.reshape(2, 2 * n, N) if dp_ else q.reshape(2 * n, N)
    x["tx"] = tx if dp_ else tx[0]
    return _freeze(x)


PLANTED_KINDS = ("posterior-tie", "off-grid", "subnormal", "pmf-zeros", "pmf-one-level")
PLANTED_DP = {f"{k}-n{n}": (k, n) for k in PLANTED_KINDS for n in (2, 4, 8)}
PLANTED_AWGN = dict(PLANTED_DP)
DP_TIES = {"tie-1-3-n8": (1, 3, 8), "tie-2-5-n8": (2, 5, 8), "tie-3-6-n4": (3, 6, 4)}       # two with a flipped hypothesis (h >= 4)
AWGN_TIES = {"tie-1-2-n8": (1, 2, 8), "tie-2-3-n4": (2, 3, 4)}


@functools.lru_cache(maxsize=None)
def planted_dp(name):
    """-> (x, the q-mode model's result)."""
    if name in DP_TIES:
        return _tie_dp(*DP_TIES[name], seed0=71000)
    kind, n = PLANTED_DP[name]
    x = _plant("dp", kind, n, 70000 + 10 * n)
    return x, I.info_q(x["q"], x["tx"], x["P"], x["shift"], x["r"], None)


@functools.lru_cache(maxsize=None)
def planted_awgn(name):
    if name in AWGN_TIES:
        return _tie_awgn(*AWGN_TIES[name], seed0=73000)
    kind, n = PLANTED_AWGN[name]
    x = _plant("awgn", kind, n, 72000 + 10 * n)
    return x, A.info_q(x["q"], x["tx"], x["P"], x["shift"])


def format_bounds(z, n, K):
    """What float32 can hold of a y-mode figure whose exponents are huge: z[..., n, K'] the float64 model's exponents in bit of the kept symbols'
    axes.  A symbol's AIR term is a difference of two floats of magnitude max_i |z_i| and its GMI term one of two of b = log2 n times that; each
    is good to half a float32 spacing at best -> (AIR bound, GMI bound) in bit: the sum of those half spacings over the K kept symbols' mean."""
    zmax = np.abs(z).max(-2).reshape(-1)
    half = lambda v: float((np.spacing(v.astype(np.float32)).astype(np.float64) / 2).sum()) / K
    return half(zmax), half(zmax * int(round(np.log2(n))))


@functools.lru_cache(maxsize=None)
def far_dp(n):
    """y-mode far from the grid: var = 1e-6 and |y| = 50 on PLANTED_POS, the sign that of the transmitted outer level the positions are given ->
    (x, my).  Every decision there is the outer level; the exponent is of the order of 1e9 bit and stays finite."""
    N, S = 60, n - 1
    x = dict(I.make_run(seed=74000 + n, N=N, n=n, shift=(0, 0), r=0, hyp=0, batch_len=None, nu=0.0, var=(1e-6, 1e-6), n_err=(0, 0)))
    y, tx = x["y"].copy(), x["tx"].copy()
    for k, pos in enumerate(PLANTED_POS):
        for p in range(2):
            for c in range(2):
                top = (k + p + c) % 2
                tx[p, c, pos] = x["amp"][S if top else 0].astype(F16)
                y[p, c, pos] = 50.0 if top else -50.0
    x["y"], x["tx"] = y, tx
    _freeze(x)
    m = I.info_y(y, tx, x["P"], x["amp"], x["nu_sc"], x["var"], x["shift"], 0, None)
    a = x["amp"].astype(np.float64)
    z = -(y.astype(np.float64)[:, :, None, :] - a[None, None, :, None]) ** 2 / (2 * 1e-6) * np.log2(np.e)
    m["format_bounds"] = format_bounds(z[0][..., 11:49], n, 38)                # (per polarisation; both are planted alike)
    return x, m


@functools.lru_cache(maxsize=None)
def far_awgn(n):
    """far_dp for the AWGN pair, whose demapper normalises each component by its mean |y| over the whole row: |y_0| = 50 gains on PLANTED_POS, the
    magnitude of y_1 there (about 50 gains as well) and amp_mean chosen so that both components' scales stay the inverse of their gains, and every
    other sample stays on the grid -> (x, my)."""
    N, S = 60, n - 1
    x = dict(A.make_run(seed=75000 + n, N=N, n=n, shift=0, hyp=0, nu=0.0, var=1e-6, n_err=0))
    y, tx, pos = x["y"].astype(np.float64), x["tx"].copy(), list(PLANTED_POS)
    g0, g1 = A.GAINS
    top = np.array([[(k + c) % 2 for k in range(len(pos))] for c in range(2)])
    tx[:, pos] = x["amp"][np.where(top, S, 0)].astype(F16)
    rest = np.abs(y).sum(1) - np.abs(y[:, pos]).sum(1)                          # the sums of |y_c| without the planted positions
    f0 = 50.0 * g0
    amp_mean = (rest[0] + len(pos) * f0) / N / g0                              # scale_0 = amp_mean / m_0 = 1 / g0
    f1 = (amp_mean * g1 * N - rest[1]) / len(pos)                              # ... and scale_1 = 1 / g1
    y[0, pos], y[1, pos] = np.where(top[0], f0, -f0), np.where(top[1], f1, -f1)
    x.update(y=y.astype(np.float32), tx=tx, amp_mean=np.float32(amp_mean))
    _freeze(x)
    m = A.info_y(x["y"], tx, x["P"], x["amp"], x["amp_mean"], x["var"], 0)
    z = -(A.normalised(x["y"], x["amp_mean"])[:, None, :] - x["amp"].astype(np.float64)[None, :, None]) ** 2 / 1e-6 * np.log2(np.e)
    m["format_bounds"] = format_bounds(z[..., 11:49], n, 38)
    return x, m
