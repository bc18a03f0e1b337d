"""vaeq_cma (CMA / CMAbatch / CMAflex) and vaeq_cpe over their whole envelope, against the float64 restatement of tests/_ref_cma.py:
every tap count on both sides of the M <= 32 split, 1 to 4 samples per symbol, frames that sps does not divide, outputs on both sides of
the 64-symbol store flush, the four cma_kernel<HALF, STAGE> instantiations in both modes and the dispatch edges between them, batches of
distinct runs, and the CPE's chunked moving average, unwrap count and LDS ceiling."""
import numpy as np
import pytest
import torch

import oracle
from _ref_cma import cma as ref_cma, cma_frame, cma_symbol_indices, conditioned_cpe_frame, cpe as ref_cpe, envelope_shapes
from conftest import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("CMA", "CMAbatch", "CMAflex")
KERNELS = {(half, stage): f"vaeq::cma_kernel<{'true' if half else 'false'}, {'true' if stage else 'false'}>"
           for half in (True, False) for stage in (True, False)}
STATS = {}


def _note(key, value):
    STATS[key] = max(STATS.get(key, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(STATS):
        print(f"  {k}: {STATS[k]:.3g}")


def run(frames, lr, sps, mode, bl=100, st=10, want_e=True):
    """frames = [(rx, h0)] of one shape -> (out[R], h[R], e[R] or None, kernel name) from one vaeq_cma call."""
    from vae_equalizer_amd import _native as nat
    from vae_equalizer_amd.engine import cma
    rx = torch.from_numpy(np.stack([f[0] for f in frames])).to(DEV)
    h = torch.from_numpy(np.stack([f[1] for f in frames])).contiguous().to(DEV)
    lr_t = torch.tensor(np.broadcast_to(np.asarray(lr, np.float32), (len(frames),)).copy(), device=DEV)
    out, e = cma(rx, h, lr_t, sps, mode, bl, st, want_e=want_e)
    torch.cuda.synchronize()
    return out.cpu().numpy(), h.cpu().numpy(), None if e is None else e.cpu().numpy(), nat.last_kernel()


def _batch_params(K):
    return max(4, min(30, K - 4)), 3


# ------------------------------------------------------------------ FIR and index mapping (lr = 0)
@pytest.mark.parametrize("mode", MODES)
def test_fir_and_index_lr0(mode):
    """lr = 0 in every mode over the (M, sps, N) grid: the output and error of every symbol land where the reference puts them, and h comes
    back bit for bit (mode 1 still runs the ring and the update sums; an added 0 * NaN would show)."""
    seen = set()
    for i, (M, sps, N) in enumerate(envelope_shapes()):
        rx, h0 = cma_frame(1000 + i, N, sps, M)
        bl, st = _batch_params(N // sps)
        out, h, e, name = run([(rx, h0)], 0.0, sps, mode, bl, st)
        seen.add(name)
        ro, _, re_ = ref_cma(rx, h0, 0.0, sps, mode, bl, st)
        assert np.array_equal(h[0], h0), (M, sps, N)
        eo, ee = relerr(out[0], ro), relerr(e[0], re_)
        _note("lr0 out relerr", eo)
        _note("lr0 e relerr", ee)
        assert eo < 2e-6 and ee < 2e-6, (M, sps, N, eo, ee)
    stage = mode == "CMAflex"                  # (symb_step 3: staged wherever batchlen >= 12; CMAbatch has symb_step = batchlen, never staged)
    assert seen >= {KERNELS[(True, stage)], KERNELS[(False, stage)]}, seen


# ------------------------------------------------------------------ training (lr > 0), every instantiation in each of its modes
TRAIN = [  # M, sps, N, mode, lr, batchlen, symb_step, instantiation (HALF, STAGE)
    (25, 2, 2000, "CMA", 5e-4, 100, 10, (True, False)),
    (31, 3, 3001, "CMA", 5e-4, 100, 10, (True, False)),
    (1, 4, 1200, "CMA", 5e-4, 100, 10, (True, False)),
    (41, 1, 1500, "CMA", 3e-4, 100, 10, (False, False)),
    (63, 4, 4002, "CMA", 2e-4, 100, 10, (False, False)),
    (25, 2, 2000, "CMAbatch", 1e-4, 100, 100, (True, False)),
    (33, 3, 2999, "CMAbatch", 1e-4, 50, 50, (False, False)),
    (31, 2, 2000, "CMAflex", 5e-5, 40, 10, (True, True)),
    (25, 2, 2000, "CMAflex", 5e-5, 30, 7, (True, True)),
    (3, 1, 1000, "CMAflex", 1e-4, 12, 2, (True, True)),
    (41, 2, 1800, "CMAflex", 2e-5, 100, 10, (False, True)),
    (63, 1, 1500, "CMAflex", 2e-5, 64, 16, (False, True)),
    (41, 3, 3001, "CMAflex", 5e-5, 30, 10, (False, False)),                # 4 symb_step > batchlen: not staged
]


def _check_training(M, sps, N, mode, lr, bl, st, seeds, tag):
    frames = [cma_frame(s, N, sps, M) for s in seeds]
    lrs = [lr * (1 + 0.25 * i) for i in range(len(frames))]
    out, h, e, name = run(frames, lrs, sps, mode, bl, st)
    for r, (rx, h0) in enumerate(frames):
        ro, rh, re_ = ref_cma(rx, h0, lrs[r], sps, mode, bl, st)
        ho = h0.copy()
        oo, eo = oracle.cma(rx, ho, lrs[r], sps, mode, bl, st, 1.0, np.float32)     # the float32 yardstick: the same sums in float32
        assert np.abs(rh - h0).max() > 1e-3, (tag, r)                             # the taps did move
        for what, got, f32, ref in (("out", out[r], oo, ro), ("e", e[r], eo, re_), ("h", h[r], ho, rh)):
            err, base = relerr(got, ref), relerr(f32, ref)
            _note(f"train {what} relerr", err)
            _note("train err / tolerance", err / max(5e-5, 8 * base))
            _note("train err / f32-oracle err", err / max(base, 1e-30))
            assert err <= max(5e-5, 8 * base), (tag, r, what, err, base)
    return name


@pytest.mark.parametrize("M,sps,N,mode,lr,bl,st,inst", TRAIN)
def test_training_against_float64(M, sps, N, mode, lr, bl, st, inst):
    """Two runs with their own frames, taps and step sizes in one call: out, e and the final taps against float64, within 8 x what the
    same arithmetic costs in float32 (the C oracle at float32) or 5e-5."""
    name = _check_training(M, sps, N, mode, lr, bl, st, (M * 100 + sps, M * 100 + sps + 1), (M, sps, N, mode))
    assert name == KERNELS[inst], name


# ------------------------------------------------------------------ dispatch edges
@pytest.mark.parametrize("M,sps,N,bl,st,inst", [
    (25, 2, 1200, 40, 10, (True, True)),        # 4 symb_step == batchlen: staged ...
    (25, 2, 1200, 39, 10, (True, False)),       # ... one less: not
    (25, 1, 1000, 229, 10, (True, True)),       # sps (batchlen + 2) + M = 256: the ring exactly full
    (25, 1, 1000, 230, 10, (True, True)),       # 257: the next power of two
    (25, 2, 1200, 256, 10, (True, True)),       # batchlen 32 B + ring 1024 x 16 B = 24 KiB: staged ...
    (25, 2, 1200, 257, 10, (True, False)),      # ... 32 B more: not
    (41, 2, 1200, 256, 10, (False, True)),
    (41, 2, 1200, 257, 10, (False, False)),
    (25, 1, 4300, 4096, 50, (True, False)),     # 128 KiB of ring: past the 48 KiB default, through the attribute
    (63, 1, 4300, 4096, 64, (False, False)),
    (25, 2, 1200, 30, 1, (True, True)),         # an update after every symbol
    (41, 2, 1200, 30, 1, (False, True)),
    (25, 2, 1200, 10, 37, (True, False)),       # symb_step > batchlen
    (41, 2, 1200, 10, 37, (False, False)),
])
def test_dispatch_edges(M, sps, N, bl, st, inst):
    name = _check_training(M, sps, N, "CMAflex", 2e-5 if bl > 200 else 5e-5, bl, st, (7 * bl + st,), (M, sps, N, bl, st))
    assert name == KERNELS[inst], name


@pytest.mark.parametrize("mode", ["CMAbatch", "CMAflex"])
@pytest.mark.parametrize("M", [25, 41])
def test_batchlen_longer_than_the_frame(M, mode):
    """batchlen > K: no update ever fires, so h comes back bit for bit even at a large step size."""
    rx, h0 = cma_frame(11, 600, 2, M)
    out, h, e, _ = run([(rx, h0)], 1e-2, 2, mode, 305, 5)
    ro, _, re_ = ref_cma(rx, h0, 1e-2, 2, mode, 305, 5)
    assert np.array_equal(h[0], h0) and relerr(out[0], ro) < 2e-6 and relerr(e[0], re_) < 2e-6


# ------------------------------------------------------------------ the three suspected bugs
def test_m1_with_a_ragged_frame_is_refused():
    """Bug 1: M = 1, N % sps != 0 puts the last symbol at k = K (IndexError in the reference); the kernel stored one element past the run's
    out / e slice.  Now refused; M = 1 with N % sps == 0 still runs."""
    from vae_equalizer_amd import _native as nat
    for N, sps in ((129, 2), (130, 3), (4001, 4)):
        rx, h0 = cma_frame(3, N, sps, 1)
        for mode in MODES:
            with pytest.raises(nat.VaeqError, match="code -2"):
                run([(rx, h0)], 1e-3, sps, mode, 10, 5)
    rx, h0 = cma_frame(3, 128, 2, 1)
    out, _, _, _ = run([(rx, h0)], 0.0, 2, "CMA")
    assert relerr(out[0], ref_cma(rx, h0, 0.0, 2, "CMA")[0]) < 2e-6


@pytest.mark.parametrize("M,sps,N,mode", [(3, 2, 13, "CMA"), (3, 2, 13, "CMAflex"), (25, 2, 101, "CMA"), (25, 2, 101, "CMAflex"), (31, 4, 250, "CMA"),
                                          (3, 3, 100, "CMAflex"), (25, 2, 401, "CMAbatch"), (25, 3, 1201, "CMAbatch"), (41, 2, 181, "CMAflex"),
                                          (63, 4, 1003, "CMA"), (3, 3, 200, "CMAflex")])
def test_wrapped_symbol_overwritten_by_the_last(M, sps, N, mode):
    """Bug 2: with N % sps != 0 there are K + 1 symbols; symbol 0 wraps to K - joff, where the last symbol lands too, and the reference keeps
    the last.  With K < 64 both sit in one flush store (lanes 0 and K), with K >= 64 in two."""
    idx = cma_symbol_indices(N, sps, M)
    K = N // sps
    assert len(idx) == K + 1 and idx[0] == idx[-1]
    rx, h0 = cma_frame(N + M, N, sps, M)
    for lr in (0.0, 5e-5):
        out, h, e, _ = run([(rx, h0)], lr, sps, mode, 20, 4)
        ro, rh, re_, sym = ref_cma(rx, h0, lr, sps, mode, 20, 4, symbols=True)
        k = idx[-1]
        assert np.abs(sym[0] - sym[-1]).max() > 0.05                               # the two candidates differ
        got = out[0][:, 0, k] + 1j * out[0][:, 1, k]
        assert np.abs(got - sym[-1]).max() < 1e-5 * max(1.0, np.abs(sym).max()), (lr, got, sym[-1], sym[0])
        assert relerr(out[0], ro) < 5e-5 and relerr(e[0], re_) < 5e-5 and relerr(h[0], rh) < 5e-5


def test_staging_with_more_than_64_samples_per_symbol():
    """Bug 3: the ring is filled by lanes 0 .. sps - 1 only, so at sps > 64 the positions 64 .. sps - 1 of each stride were never written.
    sps = 72, M = 3, CMAflex with batchlen 4 and symb_step 1 passed every staging condition; it now takes the plain path."""
    rx, h0 = cma_frame(72, 72 * 40, 72, 3)
    for lr in (0.0, 2e-5):
        out, h, e, name = run([(rx, h0)], lr, 72, "CMAflex", 4, 1)
        ro, rh, re_ = ref_cma(rx, h0, lr, 72, "CMAflex", 4, 1)
        assert name == KERNELS[(True, False)]
        assert relerr(out[0], ro) < 5e-5 and relerr(e[0], re_) < 5e-5 and relerr(h[0], rh) < 5e-5


# ------------------------------------------------------------------ batches
@pytest.mark.parametrize("M,sps,N,mode,bl,st", [(25, 2, 1000, "CMA", 100, 10), (41, 3, 1201, "CMA", 100, 10), (25, 2, 1000, "CMAflex", 40, 10),
                                                (41, 2, 1000, "CMAflex", 40, 10), (25, 2, 1001, "CMAbatch", 50, 50), (63, 1, 900, "CMAbatch", 50, 50)])
def test_batch_of_distinct_runs_equals_single_runs(M, sps, N, mode, bl, st):
    """R = 7 runs with their own rx, h and lr in one call are bit-identical to seven R = 1 calls; e = NULL changes neither out nor h."""
    frames = [cma_frame(500 + r, N, sps, M) for r in range(7)]
    lrs = [1e-5 * (1 + r) if mode != "CMA" else 1e-4 * (1 + r) for r in range(7)]
    out, h, e, _ = run(frames, lrs, sps, mode, bl, st)
    for r in range(7):
        o1, h1, e1, _ = run([frames[r]], lrs[r], sps, mode, bl, st)
        assert np.array_equal(out[r], o1[0]) and np.array_equal(h[r], h1[0]) and np.array_equal(e[r], e1[0]), r
    out2, h2, e2, _ = run(frames, lrs, sps, mode, bl, st, want_e=False)
    assert e2 is None and np.array_equal(out2, out) and np.array_equal(h2, h)
    assert len({float(np.abs(h[r] - frames[r][1]).max()) for r in range(7)}) == 7            # seven different trajectories


# ------------------------------------------------------------------ CPE
CPE_N = [1, 2, 250, 251, 500, 501, 511, 512, 513, 1023, 1537, 3000, 9980, 12800]
KINDS = ("up", "down", "walk", "zero")


@pytest.mark.parametrize("N", CPE_N)
def test_cpe_against_float64(N):
    """Four runs in one call (a phase ramp of each sign with up to three unwraps per polarisation, a random walk, an all-zero frame) at the
    windows 1, 3, 501 and one longer than the frame, on inputs where no float32 rounding can flip a pi/2 rotation."""
    from vae_equalizer_amd import _native as nat
    from vae_equalizer_amd.engine import cpe
    for M_ma in (1, 3, 501, 2 * N + 1):
        ys = [conditioned_cpe_frame(N * 10 + M_ma, N, M_ma, kind)[2] for kind in KINDS]
        got = cpe(torch.from_numpy(np.stack(ys)).to(DEV), M_ma)
        torch.cuda.synchronize()
        assert nat.last_kernel() == "vaeq::cpe_kernel"
        got = got.cpu().numpy()
        for r, kind in enumerate(KINDS):
            if kind == "zero":
                assert not np.any(got[r]), (N, M_ma)
                continue
            err = relerr(got[r], ref_cpe(ys[r], M_ma))
            _note("cpe relerr", err)
            assert err < 2e-5, (N, M_ma, kind, err)


# ------------------------------------------------------------------ coverage
def test_every_cma_instantiation_is_reached():
    names = set()
    for M, sps, N, mode, bl, st in ((25, 2, 600, "CMA", 100, 10), (25, 2, 600, "CMAflex", 40, 10), (41, 2, 600, "CMA", 100, 10),
                                    (41, 2, 600, "CMAflex", 100, 10), (25, 2, 600, "CMAbatch", 100, 100), (41, 2, 600, "CMAbatch", 100, 100)):
        names.add(run([cma_frame(1, N, sps, M)], 1e-5, sps, mode, bl, st)[3])
    print("  reached:", sorted(names))
    assert names == set(KERNELS.values())
