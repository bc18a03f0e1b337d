"""Float64 numpy restatement of the DP constant-modulus baselines and their carrier phase estimation, written from the math of
optical_DP_channel/shared_funcs.py: CMA (:341-383), CMAbatch (:385-433), CMAflex (:435-488) and CPE (:139-186).

Test infrastructure only: nothing in the package imports it.  Layouts are the kernels' (and the reference's): rx[2][2][N] = [pol][re/im][sample],
h[2][2][2][M] = [out pol][in pol][re/im][tap], out[2][2][K], e[K][2], K = N // sps.

What it keeps from the reference, on purpose:
- the frame is zero-padded by mh = M // 2 on both sides and divided by the mean of |y_pol|^2 over the PADDED length (:346-351), a power;
- symbol j (padded centre i = mh + sps j, :355) is stored at k = i // sps - mh, which is negative for the first symbols and then wraps to the
  end of out / e like a tensor index does; a later symbol at the same index overwrites it (the last write wins);
- an index outside [-K, K) raises IndexError, as the reference's out[0,0,k] = ... does;
- CMA updates the taps after every symbol (:371-381); the batch forms apply the increments of symbols k - batchlen .. k - 1 when
  k % symb_step == 0 and k >= batchlen (CMAflex :475, CMAbatch :421 with symb_step = batchlen).  The reference's CMAbatch also fires at
  negative k = -m batchlen (it tests k != 0, not k >= batchlen); its slices then read torch.empty memory, which nothing can restate, so
  those updates are skipped here as in the kernel and the C oracle.
- eval=False computes out and e with the taps left untouched (:370, :405).

In complex notation (y_p = re + j im of input pol p, h_op likewise) the FIR is out_o = sum_p sum_t h_op[t] y_p[t] (:359-363) and the
increment of :372-380 is e_o out_o conj(y_p[t]).
"""
import numpy as np


def _cplx(a):
    """[..., 2, n] re/im planes -> complex [..., n]."""
    return a[..., 0, :] + 1j * a[..., 1, :]


def _planes(c):
    """complex [..., n] -> [..., 2, n] re/im planes."""
    return np.stack([c.real, c.imag], axis=-2)


def cma(rx, h, lr, sps=2, mode="CMA", batchlen=100, symb_step=10, R=1.0, eval=True, symbols=False):
    """One frame: rx[2,2,N], h[2,2,2,M] (not modified) -> (out[2,2,K], h_final[2,2,2,M], e[K,2]), all float64; with symbols=True also the
    complex output of every symbol in symbol order, [J][out pol], overwritten ones included."""
    rx = np.asarray(rx, np.float64)
    hc = _cplx(np.asarray(h, np.float64)).copy()                       # [out pol][in pol][tap]
    M, N = hc.shape[-1], rx.shape[-1]
    mh, K = M // 2, N // sps
    y = np.zeros((2, 2, N + 2 * mh))
    y[:, :, mh:mh + N] = rx                                            # :346-348
    y /= np.mean(y[:, 0, :] ** 2 + y[:, 1, :] ** 2)                    # :349-351 (mean over [2, N + 2 mh])
    yc = _cplx(y)                                                      # [in pol][padded sample]
    J = (N + sps - 1) // sps                                           # i = mh + sps j < N + mh (:355)
    kraw = (mh + sps * np.arange(J)) // sps - mh                       # :357
    if J and (kraw[0] < -K or kraw[-1] >= K):
        raise IndexError(f"symbol index {int(kraw[0]) if kraw[0] < -K else int(kraw[-1])} is out of bounds for {K} outputs")
    W = np.lib.stride_tricks.sliding_window_view(yc, M, axis=-1)[:, ::sps][:, :J].transpose(1, 0, 2)   # [symbol][in pol][tap]
    if mode == "CMAbatch":
        symb_step = batchlen
    elif mode != "CMAflex" and mode != "CMA":
        raise ValueError(mode)
    oc = np.empty((J, 2), complex)                                     # per symbol: complex output of both output pols
    if mode == "CMA":
        if not eval or lr == 0:
            oc[:] = np.einsum("opt,jpt->jo", hc, W)
        else:
            for j in range(J):
                o = np.einsum("opt,pt->o", hc, W[j])
                oc[j] = o
                ee = R - np.abs(o) ** 2
                hc += 2 * lr * (ee * o)[:, None, None] * np.conj(W[j])[None]
    else:
        # the taps change only at update symbols: the outputs between two updates are one product each
        upd = [j for j in range(J) if kraw[j] >= batchlen and kraw[j] % symb_step == 0] if eval else []
        lo = 0
        for j in upd:
            oc[lo:j + 1] = np.einsum("opt,jpt->jo", hc, W[lo:j + 1])
            lo = j + 1
            s = slice(j - batchlen, j)                                 # symbol number = k + joff; k - batchlen .. k - 1 are never wrapped
            o = oc[s]
            ee = R - np.abs(o) ** 2
            hc += 2 * lr * np.einsum("jo,jpt->opt", ee * o, np.conj(W[s]))
        oc[lo:] = np.einsum("opt,jpt->jo", hc, W[lo:])
    out = np.zeros((2, 2, K))
    e = np.full((K, 2), np.nan)                                        # (torch.empty in the reference; every index gets written)
    kk = np.where(kraw < 0, kraw + K, kraw)
    last = np.arange(J) + K >= J                                       # kraw grows by 1 per symbol: symbol j + K, if any, overwrites symbol j
    out[:, :, kk[last]] = _planes(oc[last].T)
    e[kk[last]] = R - np.abs(oc[last]) ** 2
    return (out, _planes(hc), e, oc) if symbols else (out, _planes(hc), e)


def cma_symbol_indices(N, sps, M):
    """Output index of every symbol (after the wrap) -- the tests use it to find overwritten and wrapped symbols."""
    mh, K = M // 2, N // sps
    kraw = (mh + sps * np.arange((N + sps - 1) // sps)) // sps - mh
    return np.where(kraw < 0, kraw + K, kraw)


def cma_frame(seed, N, sps, M):
    """4-QAM at sps samples per symbol (a triangular pulse), a fixed 2x2 polarisation mix with a little ISI, noise; taps: a perturbed Dirac
    (init(), shared_funcs.py:583-585) so that every tap takes part from the first symbol on."""
    rng = np.random.default_rng(seed)
    K = -(-N // sps)
    s = (rng.choice([-1.0, 1.0], (2, 2, K)) / np.sqrt(2)).astype(np.float64)
    up = np.zeros((2, 2, K * sps))
    up[..., ::sps] = s
    pulse = np.convolve(np.ones(sps), np.ones(sps))[sps - 1:] / sps if sps > 1 else np.ones(1)
    x = np.stack([[np.convolve(up[p, c], pulse)[:K * sps] for c in range(2)] for p in range(2)])[..., :N]
    xc = x[:, 0] + 1j * x[:, 1]
    a = np.pi / 7
    mix = np.array([[np.cos(a), np.sin(a) * np.exp(0.3j)], [-np.sin(a), np.cos(a) * np.exp(-0.2j)]])
    yc = mix @ xc
    yc[:, 1:] += 0.15 * yc[:, :-1]
    yc += 0.05 * (rng.standard_normal(yc.shape) + 1j * rng.standard_normal(yc.shape))
    rx = np.stack([yc.real, yc.imag], axis=1).astype(np.float32)
    h0 = (0.01 * rng.standard_normal((2, 2, 2, M))).astype(np.float32)
    h0[0, 0, 0, M // 2] += 1
    h0[1, 1, 0, M // 2] += 1
    return rx, h0


def cpe_phase(y, M_ma=501):
    """The raw (not unwrapped) phase estimate of both polarisations [2][N] and the 4th-power moving averages [2][2][N] it comes from."""
    y = np.asarray(y, np.float64)
    a, b = y[:, 0], y[:, 1]
    a2, b2 = a * a, b * b
    p4 = np.stack([a2 * a2 - 6 * a2 * b2 + b2 * b2, 4 * (a2 * a * b - a * b2 * b)], axis=1)         # (a + jb)^4 (:150-154)
    half = M_ma // 2
    pad = np.pad(p4, ((0, 0), (0, 0), (half, half)))
    ker = np.full(M_ma, 1.0 / M_ma)
    ma = np.stack([[np.convolve(pad[p, c], ker, mode="valid") for c in range(2)] for p in range(2)])    # zero-padded moving average (:157-160)
    return np.arctan2(ma[:, 1], -ma[:, 0]) / 4, ma                                                   # :162


def cpe(y, M_ma=501):
    """y[2,2,N] -> phase-corrected y (float64).  Sample n is corrected by -pi/2 per upward jump (> pi/4) of the raw phase before it and by
    +pi/2 per downward jump (:163-168), then de-rotated (:179-184)."""
    y = np.asarray(y, np.float64)
    phi, _ = cpe_phase(y, M_ma)
    d = np.diff(phi, axis=-1)
    jumps = (d < -np.pi / 4).astype(np.float64) - (d > np.pi / 4)
    phi = phi + np.pi / 2 * np.concatenate([np.zeros((2, 1)), np.cumsum(jumps, axis=-1)], axis=-1)
    cs, sn = np.cos(phi), np.sin(phi)
    a, b = y[:, 0], y[:, 1]
    return np.stack([a * cs - b * sn, b * cs + a * sn], axis=1)


def cpe_conditioned(y, M_ma=501, margin=1e-3):
    """True when one float32 rounding cannot flip a whole pi/2 rotation of the CPE output: no raw phase step |dphi| within `margin` of pi/4,
    no averaged 4th-power angle within `margin` of +-pi (where atan2 changes branch), and no average that cancels to almost nothing."""
    phi, ma = cpe_phase(y, M_ma)
    ang = np.arctan2(ma[:, 1], -ma[:, 0])
    d = np.abs(np.diff(phi, axis=-1))
    y = np.asarray(y, np.float64)
    half = M_ma // 2
    p4 = np.pad((y[:, 0] ** 2 + y[:, 1] ** 2) ** 2, ((0, 0), (half, half)))
    tot = np.stack([np.convolve(p4[p], np.full(M_ma, 1.0 / M_ma), mode="valid") for p in range(2)])   # the same window over |y|^4
    return bool(np.all(np.abs(d - np.pi / 4) > margin) and np.all(np.pi - np.abs(ang) > margin)
                and np.all(np.hypot(ma[:, 0], ma[:, 1]) > 0.05 * tot))


def cpe_frame(seed, N, M_ma, kind, q=64):
    """A CPE test frame y[2,2,N] (float32): 4-QAM (|s|^4 = 1 at unit amplitude) with noise and a carrier phase of the given kind, quantised
    to multiples of 1/q (exact in float32, int8 codes for q = 64).
      "up" / "down": a linear ramp over the middle of the frame, steep enough that the averaged 4th-power angle steps by >= 4e-3 per symbol
                     near its +-pi crossings, flat enough that one window turns it by less than 4 rad (no cancelling average); up to three
                     crossings, i.e. unwraps, where the frame is long enough.
      "walk": a small random walk around a fixed phase (no crossings).
      "zero": an all-zero frame."""
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros((2, 2, N), np.int8), np.zeros((2, 2, N), np.float32)
    n = np.arange(N)
    if kind == "walk":
        phi = rng.uniform(-0.4, 0.4) + np.cumsum(rng.standard_normal(N)) * (0.3 / np.sqrt(max(N, 1)))
    else:
        w = min(M_ma, N)
        slope = min(1.0 / w, 0.1)                                     # phase per symbol: 4 slope w <= 4 rad per window
        length = min(N, int(np.ceil(3 * (np.pi / 2) / slope)))        # three pi/2 steps of phi at most
        start = (N - length) // 2
        ramp = np.clip(n - start, 0, length) * slope * (1 if kind == "up" else -1)
        phi = rng.uniform(-np.pi / 4, np.pi / 4) + ramp
    s = (rng.choice([-1.0, 1.0], (2, N)) + 1j * rng.choice([-1.0, 1.0], (2, N))) / np.sqrt(2) * np.exp(1j * phi)
    s += 0.03 * (rng.standard_normal((2, N)) + 1j * rng.standard_normal((2, N)))
    codes = np.clip(np.round(np.stack([s.real, s.imag], axis=1) * q), -127, 127).astype(np.int8)
    return codes, codes.astype(np.float32) / np.float32(q)


def conditioned_cpe_frame(seed, N, M_ma, kind, tries=400):
    """The first frame from seed, seed + 1, ... that cpe_conditioned() accepts (all-zero frames need no search)."""
    for s in range(seed, seed + tries):
        codes, y = cpe_frame(s, N, M_ma, kind)
        if kind == "zero" or cpe_conditioned(y, M_ma):
            return s, codes, y
    raise RuntimeError(f"no conditioned CPE frame for N={N} M_ma={M_ma} {kind} in {tries} seeds")


def envelope_shapes():
    """(M, sps, N) of the FIR / index grid: M in {1, 3, 25, 31, 33, 41, 63} (both sides of the M <= 32 split and the 63-tap limit) x
    sps in {1, 2, 3, 4} x K = N // sps in {2M, 63, 64, 65, 211} (the store flush of 64 symbols on both sides; K >= 2M, the host limit),
    each with N % sps == 0 and, for sps > 1, != 0 -- except where the reference raises IndexError (M = 1, N % sps != 0)."""
    shapes = []
    for M in (1, 3, 25, 31, 33, 41, 63):
        for sps in (1, 2, 3, 4):
            for K in sorted({2 * M, 63, 64, 65, 211}):
                if K < 2 * M:
                    continue
                for rem in sorted({0, sps - 1, (sps - 1) // 2 + 1} if sps > 1 else {0}):
                    if rem and M == 1:
                        continue
                    shapes.append((M, sps, K * sps + rem))
    return shapes
