"""CPU checks of the float64 restatement of the DP constant-modulus baselines and CPE (tests/_ref_cma.py) -- the yardstick of
test_cma_envelope_gpu.py -- against the reference's own outputs (G12, G17) and the float64 C oracle, and the host-side refusals of
vaeq_cma / vaeq_cpe (no GPU is touched: every call is refused before a pointer is used)."""
import ctypes as C

import numpy as np
import pytest

import oracle
from _ref_cma import cma, cma_frame, conditioned_cpe_frame, cpe, envelope_shapes
from conftest import load_golden, relerr

MODES = ("CMA", "CMAbatch", "CMAflex")


# ------------------------------------------------------------------ against the reference (float32 torch) captures
@pytest.mark.parametrize("tag,mode", [("cma", "CMA"), ("cmabatch", "CMAbatch"), ("cmaflex", "CMAflex")])
def test_restatement_against_G12(tag, mode):
    g = load_golden("G12_cma")
    out, h, e = cma(g["rx"], g["h0"], float(g[f"lr_{tag}"]), int(g["sps"]), mode, int(g["batchlen"]), int(g["symb_step"]))
    assert relerr(out, g[f"{tag}_out"]) < 5e-6 and relerr(e, g[f"{tag}_e"]) < 5e-6 and relerr(h, g[f"{tag}_h"]) < 5e-6


@pytest.mark.parametrize("name", ["G17_cma_m41_flex_sps2", "G17_cma_m63_sps1", "G17_cma_m25_batch_sps3", "G17_cma_flex_step7"])
def test_restatement_against_G17(name):
    g = load_golden(name)
    out, h, e = cma(g["rx"], g["h0"], float(g["lr"]), int(g["sps"]), str(g["mode"]), int(g["batchlen"]), int(g["symb_step"]))
    assert relerr(out, g["out"]) < 5e-6 and relerr(e, g["e"]) < 5e-6 and relerr(h, g["h"]) < 5e-6
    assert np.abs(g["h"] - g["h0"]).max() > 1e-2                              # the taps did move
    rx, h0 = cma_frame(int({"G17_cma_m41_flex_sps2": 171, "G17_cma_m63_sps1": 172, "G17_cma_m25_batch_sps3": 173,
                            "G17_cma_flex_step7": 174}[name]), g["rx"].shape[-1], int(g["sps"]), int(g["M"]))
    assert np.array_equal(rx, g["rx"]) and np.array_equal(h0, g["h0"])      # the tests' frame generator made these frames


def test_G17_double_write_is_last_write_wins():
    """N = 1201 at sps = 3, M = 25: symbol 0 wraps to k = -8 -> 392 and the last symbol (j = 400) lands on 392 as well; the reference keeps
    the last symbol's output there, and the two differ by far more than the tolerance."""
    g = load_golden("G17_cma_m25_batch_sps3")
    _, _, _, sym = cma(g["rx"], g["h0"], float(g["lr"]), 3, "CMAbatch", int(g["batchlen"]), symbols=True)
    assert g["rx"].shape[-1] == 1201 and len(sym) == 401
    got = g["out"][:, 0, 392] + 1j * g["out"][:, 1, 392]
    assert np.abs(got - sym[400]).max() < 1e-5 and np.abs(got - sym[0]).max() > 0.05


@pytest.mark.parametrize("name", ["G17_cpe_n300", "G17_cpe_n12800"])
def test_cpe_restatement_against_G17(name):
    g = load_golden(name)
    y = g["codes"].astype(np.float32) / np.float32(g["scale"])
    N = y.shape[-1]
    seed, codes, _ = conditioned_cpe_frame(int(g["seed"]), N, 501, "up" if N == 300 else "down", tries=1)
    assert np.array_equal(codes, g["codes"])
    got = cpe(y)[..., g["idx"]]
    assert relerr(got, g["out"]) < 5e-6
    assert np.abs(g["out"] - y[..., g["idx"]]).max() > 0.3                  # a real de-rotation


def test_cpe_restatement_against_G12():
    g = load_golden("G12_cma")
    assert relerr(cpe(g["cpe_in"]), g["cpe_out"]) < 5e-6
    assert relerr(cpe(g["cpe_in"][..., ::-1]), oracle.cpe(g["cpe_in"][..., ::-1])) < 1e-9


# ------------------------------------------------------------------ against the float64 C oracle at the envelope shapes
@pytest.mark.parametrize("mode", MODES)
def test_restatement_against_f64_oracle_lr0(mode):
    """The FIR / index grid of the GPU envelope test with lr = 0 (and eval=False, which must agree with it)."""
    for i, (M, sps, N) in enumerate(envelope_shapes()):
        rx, h0 = cma_frame(1000 + i, N, sps, M)
        bl, st = (max(4, min(30, N // sps - 4)), 3)
        out, h, e = cma(rx, h0, 0.0, sps, mode, bl, st)
        out2, h2, e2 = cma(rx, h0, 1e-3, sps, mode, bl, st, eval=False)
        assert np.array_equal(out, out2) and np.array_equal(h, h2) and np.array_equal(e, e2)
        ho = h0.astype(np.float64).copy()
        oo, eo = oracle.cma(rx, ho, 0.0, sps, mode, bl, st, 1.0, np.float64)
        assert np.array_equal(ho, h0.astype(np.float64)) and np.array_equal(h, ho), (M, sps, N)
        assert relerr(out, oo) < 1e-9 and relerr(e, eo) < 1e-9, (M, sps, N)


@pytest.mark.parametrize("mode,lr,bl,st", [("CMA", 5e-4, 0, 0), ("CMAbatch", 2e-4, 20, 20), ("CMAflex", 5e-5, 30, 7), ("CMAflex", 5e-5, 8, 2),
                                           ("CMAflex", 1e-4, 12, 13)])
def test_restatement_against_f64_oracle_training(mode, lr, bl, st):
    for i, (M, sps, N) in enumerate(s for s in envelope_shapes() if s[2] // s[1] >= 64):
        rx, h0 = cma_frame(2000 + i, N, sps, M)
        out, h, e = cma(rx, h0, lr, sps, mode, bl, st)
        ho = h0.astype(np.float64).copy()
        oo, eo = oracle.cma(rx, ho, lr, sps, mode, bl, st, 1.0, np.float64)
        assert np.abs(h - h0).max() > 1e-4, (M, sps, N)
        assert relerr(out, oo) < 1e-9 and relerr(e, eo) < 1e-9 and relerr(h, ho) < 1e-9, (M, sps, N)


def test_index_error_where_the_reference_raises_one():
    """M = 1 with N % sps != 0: the last symbol lands at k = N // sps (IndexError in the reference); the oracle refuses it too."""
    rx, h0 = cma_frame(5, 129, 2, 1)
    for mode in MODES:
        with pytest.raises(IndexError):
            cma(rx, h0, 1e-3, 2, mode, 10, 5)
        with pytest.raises(IndexError):
            oracle.cma(rx, h0.astype(np.float64).copy(), 1e-3, 2, mode, 10, 5, 1.0, np.float64)
    cma(rx[..., :128], h0, 1e-3, 2, "CMA")                                   # N % sps == 0 is fine


@pytest.mark.parametrize("N", [1, 2, 250, 251, 500, 501, 511, 512, 513, 1023, 1537, 3000, 9980, 12800])
def test_cpe_restatement_against_oracle(N):
    """The oracle's np.convolve(mode="same") is the zero-padded moving average only while M_ma <= N."""
    for M_ma in (1, 3, 501, 2 * N + 1):
        if M_ma > N:
            continue
        for kind in ("up", "down", "walk", "zero"):
            _, _, y = conditioned_cpe_frame(N * 10 + M_ma, N, M_ma, kind)
            assert np.max(np.abs(cpe(y, M_ma) - oracle.cpe(y, M_ma))) < 1e-9 * max(1.0, np.abs(y).max())


# ------------------------------------------------------------------ host-side refusals
def _dummy():
    return C.c_void_p(16)         # never dereferenced: only passed next to a NULL pointer, which is refused before any launch


def test_vaeq_cma_host_side_refusals():
    from vae_equalizer_amd import _native as nat
    L = nat.lib()
    null = [None] * 5

    def call(R=1, N=4000, sps=2, M=25, mode=1, batchlen=100, symb_step=10, ptrs=null):
        """Shapes are checked before pointers, so a refused shape answers -2 even with NULL pointers, an accepted one -1."""
        p = ptrs
        return L.vaeq_cma(R, N, sps, M, mode, batchlen, symb_step, p[0], 1.0, p[1], p[2], p[3], p[4], None)

    assert call(M=24) == -2 and call(M=0) == -2 and call(M=65) == -2 and call(M=-1) == -2
    assert call(N=2 * 49, M=25) == -2 and call(N=2 * 50 - 1, M=25) == -2    # N / sps < 2M
    assert call(N=0) == -2 and call(sps=0) == -2 and call(R=-1) == -2
    assert call(N=0x20000000) == -2                                           # 4 N must fit an int (the power loop)
    assert call(mode=2) == -2 and call(mode=-1) == -2
    assert call(batchlen=0) == -2 and call(batchlen=4097) == -2 and call(symb_step=0) == -2
    assert call(M=1, N=129, sps=2, mode=0) == -2 and call(M=1, N=130, sps=3, mode=1) == -2    # the last symbol past the end (IndexError)
    assert call(ptrs=null) == -1 and call(M=1, N=128, sps=2, ptrs=null) == -1 and call(M=63, N=126, sps=1, ptrs=null) == -1
    assert call(mode=0, batchlen=0, symb_step=0, ptrs=null) == -1             # plain CMA ignores the batch parameters
    assert call(batchlen=4096, N=2 * 4200, ptrs=null) == -1
    for i in range(4):                                                        # each required pointer on its own (e may be NULL)
        q = [_dummy()] * 4 + [None]
        q[i] = None
        assert call(ptrs=q) == -1, i
    assert call(R=0, ptrs=null) == 0                                          # an empty batch is a no-op


def test_vaeq_cpe_host_side_refusals():
    from vae_equalizer_amd import _native as nat
    L = nat.lib()
    d = _dummy()
    assert L.vaeq_cpe(1, 12801, 501, None, None, None) == -2                  # three N-float tracks in LDS: N <= 12 800
    assert L.vaeq_cpe(1, 3000, 500, None, None, None) == -2 and L.vaeq_cpe(1, 3000, 0, None, None, None) == -2
    assert L.vaeq_cpe(1, 3000, -1, None, None, None) == -2 and L.vaeq_cpe(-1, 3000, 501, None, None, None) == -2
    assert L.vaeq_cpe(1, 12800, 501, None, None, None) == -1 and L.vaeq_cpe(1, 1, 1, d, None, None) == -1
    assert L.vaeq_cpe(1, 3000, 501, None, d, None) == -1
    assert L.vaeq_cpe(0, 3000, 501, None, None, None) == 0 and L.vaeq_cpe(1, 0, 501, None, None, None) == 0
