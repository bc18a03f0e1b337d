"""vaeq_tpc_bch_decode through engine.tpc_decode with a ProductCode of two EbchCodes against model (1) of tests/_ref_ebch.py, bit for bit:
out[R, C, 8], both tensors of the stream, ext (as bit patterns) and half_err with np.array_equal, no tolerance.  The cases are
tests/_ebch_cases.py's: 10 x 16, (16, 7)^2, (32, 21)^2, 65 x 64 (just above the 4096-bit boundary of the wave count), 256 x 17 (m = 8 by m = 5:
two sets of field tables, four lane slots along the columns) and the extended (128, 113)^2 block, which is the largest state and the launch above
64 KiB (one set of tables); patterns 0, 1, 4 and 6, iters 1, 2 and 4, w in {1, 4, 12}, t0 in {0, 5}, a clip that clamps r, W' and beta, a scale
per run and none, ties, a NaN, +-0 and +-inf, loud wrong bits around the used span.  Then more blocks than the launch has workgroups, two calls
against each other with the optional outputs absent, the defaults, and scale == NULL at the C ABI."""
import numpy as np
import pytest
import torch

import _ebch_cases as K
import _ref_ebch as E
import _ref_tpc as T

pytestmark = pytest.mark.gpu

FIGS = ("iters", "ok", "bit_err", "pre_err", "erased", "pay_err", "nstat2", "nbeta")
EXTRA = {"stream", "ext", "half_err"}


def _code(case):
    from vae_equalizer_amd.engine import EbchCode, ProductCode
    c1, c2 = K.CODES[case.col], K.CODES[case.row]
    code = ProductCode(EbchCode(c1.m, c1.n, bool(c1.ext)), EbchCode(c2.m, c2.n, bool(c2.ext)))
    assert code.bch and (code.n, code.k) == (c1.n * c2.n, c1.k * c2.k)
    return code


def _run(case, llr, bits, **over):
    from vae_equalizer_amd.engine import tpc_decode
    alpha, beta = K.schedules(case)
    scale = K.scale_of(case, llr)
    kw = dict(t0=case.t0, blocks=case.C, iters=case.iters, patterns=case.p, alpha=alpha, beta=beta, clip=case.clip, payload=(case.K1, case.K2),
              scale=torch.ones(case.R, device="cuda") if scale is None else torch.from_numpy(scale).cuda(), want_stream=True, want_ext=True,
              want_profile=True)
    kw.update(over)
    ret = tpc_decode(torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda(), _code(case), **kw)
    torch.cuda.synchronize()
    return ret


def _out(ret):
    return np.stack([ret[k].cpu().numpy() for k in FIGS], -1)


def _check(ret, want, n, Kp, tag):
    out, s_llr, s_bits, ext, half, _ = want
    got = _out(ret)
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
    assert np.array_equal(g_llr[:, 0], s_llr) and np.array_equal(g_bits[:, 0], s_bits)
    assert np.array_equal(g_ext.view(np.uint32), ext.view(np.uint32))
    for k, v in T.figures(out, n, Kp).items():
        assert np.array_equal(ret[k].cpu().numpy(), v), k


def _sizes(case):
    return K.CODES[case.col].n * K.CODES[case.row].n, case.K1 * case.K2


@pytest.mark.parametrize("case", K.TPC + K.TPC_LARGE + K.TPC_TINY[-1:], ids=lambda c: c.name)
def test_tpc_bch_matches_model(case):
    llr, bits = K.tpc_tensors(case)
    _check(_run(case, llr, bits), K.tpc_expected(case), *_sizes(case), case.name)


def test_grid_stride():
    case = K.TPC_STRIDE
    llr, bits = K.tpc_tensors(case)
    _check(_run(case, llr, bits), K.tpc_expected(case), *_sizes(case), case.name)


@pytest.mark.parametrize("case", [K.TPC[i] for i in (2, 7, 9, 12, 18)] + [K.TPC_LARGE[0]], ids=lambda c: c.name)
def test_repeatable_and_outputs_optional(case):
    llr, bits = K.tpc_tensors(case)
    a, b, c = _run(case, llr, bits), _run(case, llr, bits), _run(case, llr, bits, want_stream=False, want_ext=False, want_profile=False)
    assert not EXTRA & set(c) and set(a) - set(c) == EXTRA
    assert np.array_equal(_out(a), _out(b)) and np.array_equal(_out(a), _out(c))
    for k in ("llr", "bits"):
        assert torch.equal(a["stream"][k], b["stream"][k])
    assert torch.equal(a["ext"].view(torch.int32), b["ext"].view(torch.int32)) and torch.equal(a["half_err"], b["half_err"])
    for k in c:
        assert torch.equal(a[k], c[k]) if torch.is_tensor(c[k]) else a[k] == c[k], k


def test_defaults():
    from vae_equalizer_amd.engine import tpc_decode
    case = next(c for c in K.TPC if c.w == 4 and c.col == "x10")       # three spare symbols behind the C blocks: no further block fits
    llr, bits = K.tpc_tensors(case)
    code = _code(case)
    fit = (llr.shape[-1] - case.t0) * case.w // code.n
    assert fit == case.C and (code.col.k, code.row.k) == (1, 7)
    ret = tpc_decode(torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda(), code, t0=case.t0, want_stream=True, want_ext=True, want_profile=True)
    finite = np.where(np.isfinite(llr), np.abs(llr), np.float32(0.0))
    scale = ret["scale"].cpu().numpy()
    assert scale.dtype == np.float32 and np.allclose(scale, finite.reshape(case.R, -1).mean(1, dtype=np.float64), rtol=1e-5)
    assert ret["alpha"] == tuple(float(v) for v in T.schedule(T.ALPHA, 4)) and ret["beta"] == tuple(float(v) for v in T.schedule(T.BETA, 4))
    assert ret["clip"] == 2.0 ** 60
    want = E.decode_tpc(llr, bits, K.CODES[case.col], K.CODES[case.row], 4, 4, T.schedule(T.ALPHA, 4), T.schedule(T.BETA, 4), scale, T.CLIP, 1, 7,
                        case.t0, fit)
    _check(ret, want, code.n, 7, "defaults")


def test_null_scale_is_one():
    """scale == NULL at the C ABI (engine.tpc_decode always passes a tensor): the case's model ran with 1.0."""
    import ctypes as C
    from vae_equalizer_amd import _native as nat
    case = next(c for c in K.TPC if c.scale is None and c.p > 0)
    llr, bits = K.tpc_tensors(case)
    code, (alpha, beta) = _code(case), K.schedules(case)
    L, B = torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda()
    out = torch.empty(case.R, case.C, 8, dtype=torch.int32, device="cuda")
    ext = torch.empty(case.R, case.C, code.n, dtype=torch.float32, device="cuda")
    nat.check(nat.lib().vaeq_tpc_bch_decode(case.R, case.C, llr.shape[-1], case.w, case.t0, code.col.m, code.col.n, int(code.col.extended), code.row.m,
                                            code.row.n, int(code.row.extended), nat.ptr(L), nat.ptr(B, torch.int8), case.p, case.iters,
                                            alpha.ctypes.data_as(C.c_void_p), beta.ctypes.data_as(C.c_void_p), None, case.clip, case.K1, case.K2,
                                            nat.ptr(out, torch.int32), None, None, nat.ptr(ext), None, nat.current_stream(L.device)),
              "vaeq_tpc_bch_decode")
    torch.cuda.synchronize()
    want = K.tpc_expected(case)
    assert want[0][..., 7].sum() > 0                           # positions at +-beta: the scale is seen
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(ext.cpu().numpy().view(np.uint32), want[3].view(np.uint32))
