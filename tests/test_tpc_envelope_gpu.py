"""vaeq_tpc_decode over the parts of include/vaeq.h's envelope that tests/test_tpc_gpu.py leaves out, through engine.tpc_decode against model
(1) of tests/_ref_tpc.py, bit for bit: out[R, C, 8], both tensors of the stream, ext (float32 through a uint32 view: the sign of a zero
included) and half_err with np.array_equal, no tolerance.  The cases live in tests/_tpc_envelope_cases.py (its docstring lists them);
tests/test_ref_fec_envelope_host.py asserts on the CPU that the model reaches in them what this file relies on.  Every test prints its figures
before it asserts.

  the whole schedule (iters = 16: 32 half-iterations) and stops at an even h, long words along the rows (8 x 256: four lane slots on four
  waves), the smallest block (3 x 3, p = n), the wave-count boundary (65 x 64, and 256 x 17: 17 words for 16 waves), arbitrary ten-bit columns,
  the grid-stride path of the 16-wave instantiation, w in {2, 3, 5, 7, 13, 64} and a frame that fits exactly, the corners of alpha, beta and the
  scale, the two ends of the clip with planted degenerate blocks, and 40 runs of one block.

engine.tpc_decode accepts every schedule and scale used here (alpha = 16, beta = FLT_MAX, a scale tensor of any values), so all calls go through
it; the scale == NULL path of the C ABI is tests/test_tpc_gpu.py::test_null_scale_is_one's."""
import numpy as np
import pytest
import torch

import _ref_tpc as T
import _tpc_envelope_cases as E

pytestmark = pytest.mark.gpu

FIGS = ("iters", "ok", "bit_err", "pre_err", "erased", "pay_err", "nstat2", "nbeta")


def _run(case, llr, bits, blocks=None):
    from vae_equalizer_amd.engine import HammingCode, ProductCode, tpc_decode
    code = ProductCode(HammingCode(*E.CODES[case.col]), HammingCode(*E.CODES[case.row]))
    alpha, beta = E.schedules(case)
    scale = E.scale_of(case)
    ret = tpc_decode(torch.from_numpy(llr.copy()).cuda(), torch.from_numpy(bits.copy()).cuda(), code, t0=case.t0, blocks=case.C if blocks is None else blocks,
                     iters=case.iters, patterns=case.p, alpha=alpha, beta=beta, clip=case.clip, payload=(case.K1, case.K2),
                     scale=torch.ones(case.R, device="cuda") if scale is None else torch.from_numpy(scale).cuda(), want_stream=True, want_ext=True,
                     want_profile=True)
    torch.cuda.synchronize()
    return ret


def _check(ret, want, n, Kp, tag):
    out, s_llr, s_bits, ext, half, _ = want
    got = np.stack([ret[k].cpu().numpy() for k in FIGS], -1)
    g_llr, g_bits = ret["stream"]["llr"].cpu().numpy(), ret["stream"]["bits"].cpu().numpy()
    g_ext, g_half = ret["ext"].cpu().numpy(), ret["half_err"].cpu().numpy()
    short = (lambda v: v.ravel().tolist()) if out.shape[0] * out.shape[1] <= 16 else (lambda v: f"sum {int(v.sum())}")
    print(f"{tag}: half-iterations {short(out[..., 0])} ok {short(out[..., 1])} pre_err {short(out[..., 3])} post_err "
          f"{short(out[..., 2])} erased {int(out[..., 4].sum())} pay_err {int(out[..., 5].sum())} nstat2 {int(out[..., 6].sum())} nbeta "
          f"{int(out[..., 7].sum())}; out differs in {int((got != out).sum())}, stream llr in {int((g_llr[:, 0] != s_llr).sum())}, stream bits in "
          f"{int((g_bits[:, 0] != s_bits).sum())}, ext in {int((g_ext.view(np.uint32) != ext.view(np.uint32)).sum())} of {ext.size}, half_err in "
          f"{int((g_half != half).sum())}")
    assert got.dtype == np.int64 and g_llr.dtype == np.float32 and g_bits.dtype == np.int8 and g_ext.dtype == np.float32 and g_half.dtype == np.int64
    assert g_llr.shape == (out.shape[0], 1, s_llr.shape[1]) and g_bits.shape == g_llr.shape and g_ext.shape == ext.shape and g_half.shape == half.shape
    assert np.array_equal(got, out)
    assert np.array_equal(g_half, half)
    assert np.array_equal(g_llr[:, 0].view(np.uint32), s_llr.view(np.uint32)) and np.array_equal(g_bits[:, 0], s_bits)
    assert np.array_equal(g_ext.view(np.uint32), ext.view(np.uint32))
    for k, v in T.figures(out, n, Kp).items():
        assert np.array_equal(ret[k].cpu().numpy(), v), k


def _sizes(case):
    n1, n2 = E.n_of(case)
    return n1 * n2, case.K1 * case.K2


@pytest.mark.parametrize("case", [c for g in E.GROUPS for c in E.GROUPS[g]], ids=lambda c: c.name)
def test_tpc_matches_model(case):
    llr, bits = E.tensors(case)
    _check(_run(case, llr, bits), E.expected(case), *_sizes(case), case.name)


def test_grid_stride_on_sixteen_waves():
    """1027 blocks of 65 x 64 for the 1024 workgroups of the launch: three workgroups decode a second block on the LDS of their first."""
    from vae_equalizer_amd import _native as nat
    case = E.STRIDE
    n1, n2 = E.n_of(case)
    assert n1 * n2 > 4096 and nat.lib().vaeq_tpc_lds_bytes(n1, E.CODES[case.col][1], n2, E.CODES[case.row][1]) > 0
    llr, bits, want = E.stride()
    n, Kp = _sizes(case)
    _check(_run(case, llr, bits, E.STRIDE_BLOCKS), want, n, Kp, case.name)
