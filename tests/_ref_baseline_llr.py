"""Float64 numpy models of vaeq_cma_epilogue_llr and vaeq_awgn_track_llr: the per-bit a-posteriori LLRs of the constant-modulus DP baselines and
of the AWGN baselines' soft sequences, composed of what exists:

    CMA    _ref_cma_info.normalise (stage-c alignment, the mean-radius factor over W_c)  ->  _ref_llr.dp_llr_y on that sequence with the stage-q
           alignment, no per-minibatch cut: the demapper's var is the stage-c aligned row's, as in _ref_cma_info.info
    track  _ref_awgn_baseline_info.window and the scale of track_info  ->  _ref_llr.set_llr_z of -(zhat_c - a_i)^2 log2 e / var  ->
           _ref_llr.transform(., hyp & 3, n), placed at the TX indices edge + j

Test infrastructure only.  Every function returns (planes[..., 2b, N] float64, kept mask[..., N] bool); a run without a normalisation, or with an
empty window, is all zeros with nothing kept.  cma_llr32 / track_llr32 are the kernels' operation order in numpy float32: the first half of
_ref_cma_info.float32_deviation and of _ref_awgn_baseline_info.track_float32, followed by _ref_llr.set_llr_z in float32.
"""
import numpy as np

import _ref_awgn_baseline_info as T
import _ref_cma_info as C
import _ref_epilogue as E
import _ref_llr as L

# the largest |float32 emulation - float64 model| / max(1, |model|) over the kept entries of every launch of _ref_cma_info.LAUNCHES (2.205e-6, with
# |lam| up to 399 nats: the float32 fac moves the scale of every sample of W_c, and a relative error of 1e-7 in yn is one of a few 1e-6 in the
# (yn - a_i)^2 differences at 64-QAM) and of _ref_awgn_baseline_info.LAUNCHES + ["wide"] (4.292e-6, with |lam| up to 627 nats: two kept 64-QAM
# symbols, so the float32 scale is a quotient of two short sums), computed and asserted on the CPU by tests/test_ref_baseline_llr_host.py, rounded
# up, with the launch and run that sets each.  The GPU tests hold each kernel to four times its figure.
Y_LLR_DEV_CMA = 2.3e-6
Y_LLR_DEV_CMA_LAUNCH = "N400-n8 run 2"
Y_LLR_DEV_TRACK = 4.3e-6
Y_LLR_DEV_TRACK_LAUNCH = "D2-e31-dz0-il1-n8 run 1"


# ------------------------------------------------------------------ the constant-modulus DP baselines
def cma_llr(x, hyp):
    """x: a run of _ref_cma_info.make_run, hyp[2] -> (planes[2][2b][N], mask[2][N])."""
    N, n = x["y"].shape[-1], x["n"]
    yn, fac = C.normalise(x["y"], x["tx"], x["shift_c"], x["r_c"])
    if np.isnan(fac):
        return np.zeros((2, 2 * L.nbits(n), N)), np.zeros((2, N), bool)
    return L.dp_llr_y(yn, n, x["amp"], x["nu_sc"], x["var"], x["shift_q"], x["r_q"], hyp, None)


def _strided(rows, L=None):
    """The kernels' radius sum in float32, one addition at a time: thread t adds its samples t, t + 256, ... below L in index order (the rows of
    one index in turn), then -- the track kernels' tail loop -- the samples L + t, L + t + 256, ...; then the threads are added."""
    f = np.float32
    rows = np.atleast_2d(rows)
    L = rows.shape[-1] if L is None else L
    per = []
    for t in range(min(256, rows.shape[-1])):
        s = f(0)
        for v in np.concatenate([rows[:, t:L:256].T.reshape(-1), rows[:, L + t::256].T.reshape(-1)]):
            s = f(s + v)
        per.append(s)
    return np.array(per, f).sum(dtype=f) if per else f(0)


def cma_llr32(x, hyp):
    """cma_llr in numpy float32 in the kernel's operation order: fac from float32 sums of float32 radii over W_c (per thread at stride 256, both
    polarisations of an index in turn, then over the threads), the scaled sample, info_demap_log2's exponent, every bit-wise set a log-sum-exp
    around its own maximum."""
    f = np.float32
    N, n = x["y"].shape[-1], x["n"]
    ya = E.align(np.asarray(x["y"], f), x["shift_c"], x["r_c"])
    W = C.window_c(N, x["shift_c"])
    lo, hi = W.start, W.stop
    t = np.asarray(x["tx"], f)
    rt = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]).astype(f)).astype(f)
    ry = np.sqrt((ya[:, 0] * ya[:, 0] + ya[:, 1] * ya[:, 1]).astype(f)).astype(f)
    inW = (np.arange(N) >= lo) & (np.arange(N) < hi)
    st, sy = _strided(np.where(inW, rt, f(0))), _strided(np.where(inW, ry, f(0)))   # (adding the +0.0 of an index outside W_c changes no sum)
    if sy == 0:
        return np.zeros((2, 2 * L.nbits(n), N), f), np.zeros((2, N), bool)
    yn = ya.copy()
    yn[..., W] = (yn[..., W] * f(st / sy)).astype(f)
    return L.dp_llr_y(yn, n, x["amp"], x["nu_sc"], x["var"], x["shift_q"], x["r_q"], hyp, None, f)


# ------------------------------------------------------------------ the AWGN baselines' tracks
def _track_place(lam, ti, Nd, n, hyp, dtype=np.float64):
    """lam[2 axes][b][L] of the kept symbols (None: nothing to report) -> (planes[2b][Nd], mask[Nd])."""
    planes, mask = np.zeros((2 * L.nbits(n), Nd), dtype), np.zeros(Nd, bool)
    if lam is not None and len(ti):
        mask[ti] = True
        planes[:, ti] = L.transform(lam, int(hyp) & 3, n)
    return planes, mask


def track_llr(x, hyp):
    """x: a run of _ref_awgn_baseline_info.make_run, hyp -> (planes[2b][Nd], mask[Nd]): TX index edge + j holds the LLRs of sample edge + sh + j."""
    n, Nd = x["n"], x["tx"].shape[-1]
    z = np.asarray(x["z"], np.complex128)
    tx = np.asarray(x["tx"], np.float64)
    a = np.asarray(x["amp"], np.float64)
    ri, ti = T.window(len(z), Nd, x["edge"], x["shift"])
    if len(ti) == 0:
        return _track_place(None, ti, Nd, n, hyp)
    ar = np.abs(z[ri]).sum()
    if ar == 0:
        return _track_place(None, ti, Nd, n, hyp)
    scale = (np.hypot(tx[0, ti], tx[1, ti]).sum() / len(ti)) / (ar / len(ri))
    zh = z[ri[:len(ti)]] * scale
    zc = np.stack([zh.real, zh.imag])
    v = -(zc[:, None, :] - a[None, :, None]) ** 2 / float(x["var"]) * np.log2(np.e)
    return _track_place(L.set_llr_z(v, n), ti, Nd, n, hyp)


def track_llr32(x, hyp):
    """track_llr in numpy float32 in the kernel's operation order (_ref_awgn_baseline_info.track_float32's first half: the two radius sums per
    thread at stride 256 and then over the threads, scale = (at / L) / (ar / Lz), z = -(d d) (log2 e / var)), then every bit-wise set a
    log-sum-exp around its own maximum."""
    f = np.float32
    n, Nd = x["n"], x["tx"].shape[-1]
    amp = x["amp"].astype(f)
    zr, zi = x["z"].real.astype(f), x["z"].imag.astype(f)
    tx = x["tx"].astype(f)
    ri, ti = T.window(len(zr), Nd, x["edge"], x["shift"])
    K, Lz = len(ti), len(ri)
    if K == 0:
        return _track_place(None, ti, Nd, n, hyp, f)
    rad_t = np.sqrt((tx[0, ti] * tx[0, ti] + tx[1, ti] * tx[1, ti]).astype(f)).astype(f)
    rad_z = np.sqrt((zr[ri] * zr[ri] + zi[ri] * zi[ri]).astype(f)).astype(f)

    at, ar = _strided(rad_t), _strided(rad_z, K)                               # the slice's samples past the data go through the tail loop
    if ar == 0:
        return _track_place(None, ti, Nd, n, hyp, f)
    scale = f(f(at / f(K)) / f(ar / f(Lz)))
    ivl = f(f(1.4426950408889634) / f(x["var"]))
    z = np.empty((2, n, K), f)
    for c, src in enumerate((zr, zi)):
        zc = (src[ri[:K]] * scale).astype(f)
        for i in range(n):
            dd = (zc - amp[i]).astype(f)
            z[c, i] = (-(dd * dd).astype(f) * ivl).astype(f)
    return _track_place(L.set_llr_z(z, n, f), ti, Nd, n, hyp, f)
