"""Float64 numpy model of vaeq_awgn_track_info and vaeq_awgn_dfe_soft: achievable rate (AIR), generalised mutual information (GMI), NGMI and
pre-FEC BER of the AWGN baselines -- the constant-modulus script's CPE output, the LMMSE output, the DFE's slicer input -- over the symbols
their validators' SER keeps.  The reference has no such metric; the definitions are closed-form and built from pieces that exist:
tests/_ref_awgn_info.py (_figures: Gray labels, H, hypotheses, tie-break, AIR, GMI, BER; tx_levels, pmf, entropy) and tests/_ref_awgn.py (ser,
_eval_slices, dfe and the conditioned frames), imported, not edited.

Per run: a complex track z of Nz samples, TX data of Nd symbols, Nz in {Nd, Nd + 1}, edge e, shift sh.
Window: L = Nd - 2 e - sh kept symbols, Lz = Nz - 2 e - sh samples in the slice; kept symbol j < L pairs z[e + sh + j] with TX symbol e + j
(z[:, e+sh : -e] against data[:, e : -e-sh]); empty when e + sh <= 0 or L <= 0.
Normalisation (SER_CMA :73 = SER_func :117): scale = mean_{j<L} |tx_j| / mean_{m<Lz} |z[e+sh+m]| (complex radius, ALL Lz samples); zhat = z scale.
A slice whose sum of |z| is zero has no normalisation: the empty-window result.
Demapper (func_VAELE_MQAM_shaping.py:229): per axis v_i = -(zhat_c - a_i)^2 / var, posteriors = softmax of v (no 1/2, no prior term).
The DFE's soft sequence: z[p] = ff[p] + sum_{j<K2} fb[j] c(dec[p-1-j]) for p >= K2, c(i) = amp[i // n] + 1j amp[i % n]; z[p] = c(dec[p]) in front.

Test infrastructure only.  Besides the figures and counts the model returns what makes the comparison with a float32 kernel fair: `margin`, the
least distance of any normalised sample of the slice (all Lz of them, both coordinates) to a decision threshold in level spacings, `qgap`, the
smallest gap between the two largest posteriors of a kept symbol and axis, and `min_post`, the smallest posterior at a transmitted level.
"""
import functools
import itertools

import numpy as np

import _ref_awgn as R
import _ref_awgn_info as A

MARGIN_FLOOR = 0.05
QGAP_FLOOR = 0.05
MIN_POST_FLOOR = 1e-30
# bit: the largest deviation of track_float32 (the kernel's operation order in numpy float32) from the float64 model over the planted launches
# below, computed on the CPU by tests/test_ref_awgn_baseline_info_host.py (4.69e-5), rounded up.  It is set by launch Z_DEV_LAUNCH at shift 0: ONE
# kept 64-QAM symbol at var 0.004, planted wrong, whose slice holds one more sample that pulls the scale off as well -- a figure near -83 bit,
# where float32 is spaced 7.6e-6 and the exponent multiplies the rounding of the scale.  It is a property of the number format: the GPU test holds
# the kernel to three times this.  MEASURED_Z_DEV is the kernel's own largest deviation on the MI355X over the same launches (DESIGN.md
# section 5), recorded beside it and used by nothing.
Z_DEV = 5.0e-5
Z_DEV_LAUNCH = "D1-e31-dz1-il1-n8"
MEASURED_Z_DEV = 4.694e-5                                                       # the same launch and run
NU_SHAPED = A.NU_SHAPED
# The track's gain, per component.  One radius scale normalises both components, so the pair shares a common factor (the normalisation's work) and
# differs by +-1 %: neither component's gain is 1, and the imbalance -- which no scalar takes out -- moves the outermost 64-QAM level by 0.07 of
# half a level spacing, well inside the planted noise of +-0.2.
GAINS = ((0.7 * 1.01, 0.7 * 0.99), (1.9 * 0.99, 1.9 * 1.01), (1.3 * 1.01, 1.3 * 0.99))


def window(Nz, Nd, e, sh):
    """-> (track indices [Lz], TX indices [L]), both empty when the window is."""
    Nz, Nd, e, sh = int(Nz), int(Nd), int(e), int(sh)
    L = Nd - 2 * e - sh
    if e + sh <= 0 or L <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return e + sh + np.arange(L + Nz - Nd, dtype=np.int64), e + np.arange(L, dtype=np.int64)


def track_info(z, tx, P, amp, var, shift, edge):
    """z complex [Nz] (float32 values, evaluated in float64), tx[2][Nd], P[n], amp[n], var, shift, edge -> the dict of _ref_awgn_info._figures
    plus margin."""
    n = len(P)
    z = np.asarray(z, np.complex128)
    tx = np.asarray(tx, np.float64)
    a = np.asarray(amp, np.float64)
    ri, ti = window(len(z), tx.shape[-1], edge, shift)
    if len(ti) == 0:
        return A._empty()
    ar = np.abs(z[ri]).sum()
    if ar == 0:
        return A._empty()
    scale = (np.hypot(tx[0, ti], tx[1, ti]).sum() / len(ti)) / (ar / len(ri))
    zh = z[ri] * scale                                                        # all Lz normalised samples of the slice
    zc = np.stack([zh.real, zh.imag])
    v = -(zc[:, None, :len(ti)] - a[None, :, None]) ** 2 / float(var) * np.log2(np.e)
    out = A._figures(v, True, A.tx_levels(tx, n)[:, ti], P, n)
    thr = (a[1:] + a[:-1]) / 2
    out["margin"] = float(np.abs(zc[:, :, None] - thr[None, None, :]).min() / (a[1] - a[0]))
    return out


def dfe_soft(ff, fb, dec, levels):
    """ff complex [N], fb complex [K2], dec[N] indices -> z complex128 [N]."""
    lev = np.asarray(levels, np.float64)
    n, K2, N = len(lev), len(fb), len(ff)
    d = np.asarray(dec).astype(np.int64) & 0xFF
    c = lev[d // n] + 1j * lev[d % n]
    z = np.asarray(ff, np.complex128).copy()
    for j in range(K2):
        z[j + 1:] += complex(fb[j]) * c[:N - 1 - j]
    z[:K2] = c[:K2]
    return z


def dfe_soft_bound(ff, fb, dec, levels):
    """(2 K2 + 2) 2^-24 (|ff| + sum_j |fb_j| |c(dec[p-1-j])|) per sample: the roundings of the float32 sum itself (two per complex product and
    component, two to spare), each at most half a unit in the last place of a partial sum no larger than that."""
    lev = np.asarray(levels, np.float64)
    n, K2, N = len(lev), len(fb), len(ff)
    d = np.asarray(dec).astype(np.int64) & 0xFF
    c = np.abs(lev[d // n] + 1j * lev[d % n])
    s = np.abs(np.asarray(ff, np.complex128))
    for j in range(K2):
        s[j + 1:] += abs(complex(fb[j])) * c[:N - 1 - j]
    return (2 * K2 + 2) * 2.0 ** -24 * s


# ------------------------------------------------------------------ planted inputs
def feasible_errors(n, var, want):
    """Planted errors go to a NEIGHBOURING level, and only where the posterior of the transmitted level can stay above MIN_POST_FLOOR = 1e-30
    (69 nat): one spacing d with the noise of +-0.1 d costs between (0.9 d)^2 / var and (1.1 d)^2 / var nat.  64-QAM: at most 29 nat at var
    0.004.  16-QAM: at most 48 nat at 0.01; 51 .. 77 at 0.0063 (the seed search finds a planted symbol whose noise points the right way); at least
    81 at 0.004 (never).  4-QAM: at least 162 nat at 0.01 (never)."""
    if n == 8:
        return want
    if n == 4 and var >= 0.0063:
        return min(want, 2 if var >= 0.01 else 1)
    return 0


def make_run(seed, Nd, dz, e, n, shift, hyp, nu, var, n_err, gain, interleaved=True):
    """One run: TX levels from the shaped pmf, n_err of the kept symbols planted wrong by one level on one axis, the received levels un-rotated
    by hyp, at their amplitude plus up to +-0.2 of half the level spacing per coordinate, times the component's gain, rolled by +shift:
    z[m + shift] ~ tx[m].  z has Nd + dz samples (the last dz symbols have no TX partner)."""
    rng = np.random.default_rng(seed)
    amp = A.amp_levels(n)
    S, u = n - 1, float(amp[1] - amp[0]) / 2
    P = A.pmf(n, nu)
    Nz = Nd + dz
    lev = rng.choice(n, size=(2, Nz), p=P)
    tx = amp[lev[:, :Nd]].astype(np.float16)
    pool = window(Nz, Nd, e, shift)[1]
    rxl = lev.copy()
    n_err = min(n_err, len(pool))
    for pos in (rng.choice(pool, size=n_err, replace=False) if n_err else []):
        c = int(rng.integers(2))
        rxl[c, pos] += 1 if rxl[c, pos] == 0 or (rxl[c, pos] < S and rng.integers(2)) else -1
    rcv = np.stack(A.unrotate(rxl[0], rxl[1], hyp, S))
    clean = (amp[rcv].astype(np.float64) + rng.uniform(-0.2 * u, 0.2 * u, rcv.shape)) * np.asarray(gain, np.float64)[:, None]
    zz = np.roll(clean, int(shift), axis=-1).astype(np.float32)
    return dict(z=(zz[0] + 1j * zz[1]).astype(np.complex64), tx=tx, amp=amp, P=P.astype(np.float32), var=np.float32(var), shift=int(shift),
                hyp=int(hyp), n=n, n_err=n_err, seed=seed, edge=int(e), interleaved=bool(interleaved))


def model(x):
    return track_info(x["z"], x["tx"], x["P"], x["amp"], x["var"], x["shift"], x["edge"])


def meets_floors(x, m):
    """The preconditions of a fair comparison (tests/test_ref_awgn_baseline_info_host.py asserts them for every GPU case)."""
    if m["kept"] == 0:
        return True
    if not (m["margin"] >= MARGIN_FLOOR and m["qgap"] > QGAP_FLOOR and m["min_post"] >= MIN_POST_FLOOR):
        return False
    if m["kept"] >= 11:
        return m["hyp"] == x["hyp"] and m["sym_err"] == x["n_err"]
    return True


def conditioned_run(spec, tries=4000):
    """make_run(**spec) at the first seed from spec's on that meets every floor (a short slice's one extra sample, or a planted error whose noise
    points away from the transmitted level, moves a sample or a posterior past a floor: that seed is replaced by the next one, no floor is
    lowered) -> (x, m)."""
    for seed in itertools.count(spec["seed"]):
        x = make_run(**dict(spec, seed=seed))
        m = model(x)
        if meets_floors(x, m):
            return x, m
        if seed - spec["seed"] > tries:
            raise RuntimeError(f"no seed meets the floors for {spec}")


# One entry = one kernel launch of R = 3 runs with shifts -10 / 0 / +10.  D = Nd - 2 e: 1 keeps 11 / 1 / 0 symbols, 2 keeps 12 / 2 / 0, 11 keeps
# 21 / 11 / 1, 247 keeps 257 / 247 / 237 (one symbol in the second round of the 256-thread workgroup), 1008 straddles the 1000-symbol shift-search length.
DS = (1, 2, 11, 38, 247, 1008)
EDGES = (11, 31)
SHIFTS = (-10, 0, 10)
VARS = A.VARS


def _spec(D, e, dz, il, n, k, sh, base):
    i, j = DS.index(D), (2, 4, 8).index(n)
    c = i + j + EDGES.index(e) + dz + il + k
    var = VARS[c % 3]
    return dict(seed=base + 100 * k, Nd=D + 2 * e, dz=dz, e=e, n=n, shift=sh, hyp=(c + j) % 4, nu=(0.0, NU_SHAPED)[c % 2], var=var,
                n_err=feasible_errors(n, var, 1 + (i + k) % 3), gain=GAINS[(i + k) % 3], interleaved=bool(il))


@functools.lru_cache(maxsize=None)
def launches():
    L = {}
    for a, (D, e, dz, il, n) in enumerate(itertools.product(DS, EDGES, (0, 1), (0, 1), (2, 4, 8))):
        L[f"D{D}-e{e}-dz{dz}-il{il}-n{n}"] = [_spec(D, e, dz, il, n, k, sh, 50000 + 1000 * a) for k, sh in enumerate(SHIFTS)]
    return L


LAUNCHES = list(launches())
# shifts nobody clamps: find_shift_symb(., ., 24) returns -12 .. +11 (DFE_MQAM_shaping.py:292)
WIDE = [dict(seed=90000 + 100 * k, Nd=300, dz=dz, e=31, n=8, shift=sh, hyp=1 + k, nu=NU_SHAPED, var=0.0063, n_err=2, gain=GAINS[k], interleaved=True)
        for k, (sh, dz) in enumerate(((-12, 1), (11, 0), (-12, 0)))]


def _freeze(x):
    for v in x.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def build_launch(name):
    """-> (per-run inputs, per-run model results); built once, shared by the tests, never modified."""
    specs = WIDE if name == "wide" else launches()[name]
    xs, ms = [], []
    for spec in specs:
        x, m = conditioned_run(spec)
        xs.append(_freeze(x))
        ms.append(m)
    return xs, ms


def slices_of(x):
    """The track [2,Lz] and TX [2,L] slices of a run as _ref_awgn._eval_slices cuts them (None where the reference's slice is empty)."""
    Nz, Nd, e = len(x["z"]), x["tx"].shape[-1], x["edge"]
    try:
        (r0, r1), (d0, d1) = R._eval_slices(Nz, Nd, x["shift"], e - 11)
    except ValueError:
        return None
    if d1 <= d0 or r1 <= r0:
        return None
    z = x["z"].astype(np.complex128)[r0:r1]
    return np.stack([z.real, z.imag]), x["tx"].astype(np.float64)[:, d0:d1]


# ------------------------------------------------------------------ the kernel's operation order in float32
def track_float32(x, hyp):
    """vaeq_awgn_track_info's operation order in numpy float32 under hypothesis hyp: the two radius sums per thread (stride 256, index order) and
    then over the threads, scale = (at / L) / (ar / Lz), z = -(d d) (log2 e / var), the log-sum-exp of every bit-wise set around its own maximum,
    per-symbol terms, mean.  -> (AIR, GMI) as float, None when nothing is kept."""
    f = np.float32
    n, S = x["n"], x["n"] - 1
    b = int(round(np.log2(n)))
    amp = x["amp"].astype(f)
    zr, zi = x["z"].real.astype(f), x["z"].imag.astype(f)
    tx = x["tx"].astype(f)
    ri, ti = window(len(zr), tx.shape[-1], x["edge"], x["shift"])
    K, Lz = len(ti), len(ri)
    if K == 0:
        return None
    rad_t = np.sqrt((tx[0, ti] * tx[0, ti] + tx[1, ti] * tx[1, ti]).astype(f)).astype(f)
    rad_z = np.sqrt((zr[ri] * zr[ri] + zi[ri] * zi[ri]).astype(f)).astype(f)

    def strided(v):
        return np.array([v[t::256].sum(dtype=f) for t in range(min(256, len(v)))], f).sum(dtype=f)
    at, ar = strided(rad_t), strided(rad_z)
    if ar == 0:
        return None
    scale = f(f(at / f(K)) / f(ar / f(Lz)))
    ivl = f(f(1.4426950408889634) / f(x["var"]))
    z = np.empty((2, n, K), f)
    for c, src in enumerate((zr, zi)):
        zc = (src[ri[:K]] * scale).astype(f)
        for i in range(n):
            dd = (zc - amp[i]).astype(f)
            z[c, i] = (-(dd * dd).astype(f) * ivl).astype(f)
    lev = A.tx_levels(x["tx"], n)[:, ti]
    (zI, zQ), _ = A._apply(z, np.zeros((2, K), np.int64), hyp, S)
    g, H = A.gray(np.arange(n)), f(A.entropy(x["P"]))
    a, gg = np.zeros(K, f), np.zeros(K, f)
    for zz, t in ((zI, lev[0]), (zQ, lev[1])):
        def lse(mask):
            w = np.where(mask, zz, f(-np.inf)).astype(f)
            mx = w.max(0)
            return (mx + np.log2(np.exp2((w - mx).astype(f)).astype(f).sum(0, dtype=f)).astype(f)).astype(f)
        bit0 = (g & 1)[:, None]
        l0, l1 = lse(bit0 == 0), lse(bit0 == 1)
        hi, lo = np.maximum(l0, l1), np.minimum(l0, l1)
        tot = (hi + np.log2(f(1) + np.exp2((lo - hi).astype(f)).astype(f)).astype(f)).astype(f)
        a = (a + (zz[t, np.arange(K)] - tot).astype(f)).astype(f)
        gs = np.zeros(K, f)
        for k in range(b):
            gs = (gs + lse(((g >> k) & 1)[:, None] == ((g[t] >> k) & 1)[None, :])).astype(f)
        gg = (gg + (gs - f(b) * tot).astype(f)).astype(f)
    return float(f(f(2) * H + f(a.sum(dtype=f) / f(K)))), float(f(f(2) * H + f(gg.sum(dtype=f) / f(K))))


def track_float32_deviation(x, m):
    """What the float32 format costs -> largest |AIR or GMI deviation| of the run from its float64 model m in bit, None when nothing is kept."""
    r = track_float32(x, m["hyp"])
    return None if r is None else max(abs(r[0] - m["AIR"]), abs(r[1] - m["GMI"]))


# ------------------------------------------------------------------ conditioned frames through the validators
# CMA validation (vaeq_awgn_cma_validate): K, n_lev, n_shift, sps, M and three runs each (lag, rotation, injected errors, side taps)
CMA_BATCHES = [dict(K=1100, n_lev=4, n_shift=21, sps=2, M=31, branches=None,
                    runs=[dict(seed=7100 + i, lag=g, rot=i % 4, n_err=3 + i, side=0.03 if i % 2 else 0.0, gain=1.0) for i, g in enumerate((-10, 0, 10))]),
               dict(K=2100, n_lev=8, n_shift=21, sps=1, M=33, branches=None,
                    runs=[dict(seed=7200 + i, lag=g, rot=(i + 1) % 4, n_err=4 + i, side=0.03 if i % 2 else 0.0, gain=1.0) for i, g in enumerate((-7, 3, 9))])]
LMMSE_CASE = (20, 1100, 20, 21, 4)                                             # taps, N, n_cut, n_shift, n_lev (_ref_awgn.lmmse_cases' form)
DFE_CASES = [(4, 1, 1100, 9), (8, 4, 1100, 9), (8, 1, 2100, 12), (4, 4, 2100, 12)]   # n_lev, K2, N, outliers


@functools.lru_cache(maxsize=None)
def cma_batch(i):
    return R.build_validator_batch(CMA_BATCHES[i])


@functools.lru_cache(maxsize=None)
def lmmse_frames():
    """Three conditioned LMMSE frames and _ref_awgn.longer_slice_frame (the extra sample of the slice decides one symbol), one launch."""
    return [R.build_lmmse_case(LMMSE_CASE, r)[0] for r in range(3)] + [R.longer_slice_frame()]


@functools.lru_cache(maxsize=None)
def dfe_frames(case):
    n_lev, K2, N, outliers = case
    return [R.conditioned_dfe_frame(s, N, n_lev, K2, outliers) for s in R.dfe_run_seeds(n_lev, K2, N)[:2]]
