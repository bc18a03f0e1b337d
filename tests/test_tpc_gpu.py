"""vaeq_tpc_decode through engine.tpc_decode against model (1) of tests/_ref_tpc.py, bit for bit: out[R, C, 8], both tensors of the stream, ext
(as bit patterns: the floats themselves, the sign of a zero included) and half_err with np.array_equal, no tolerance -- the rule is integers and
float32 operations in a fixed order, and its one reduction over candidates is a minimum.  The cases are tests/_tpc_cases.py's (its docstring says
what they hold and tests/test_ref_tpc_host.py that they reach every branch of the rule): six blocks from 7 x 16 to the extended (128, 120)^2,
which is the largest state and the launch above 64 KiB of LDS, both wave counts, patterns 0, 1, 4 and 6, iters 1, 2 and 4, w in {1, 4, 12}, t0 in
{0, 5}, a clip that clamps, a scale per run and none, ties, a NaN, +-0 and +-inf, loud wrong bits around the used span.  Then more blocks than the
launch has workgroups, two calls against each other with the optional outputs absent, and the defaults of blocks, payload, schedules, scale and
clip."""
import numpy as np
import pytest
import torch

import _ref_tpc as T
import _tpc_cases as K

pytestmark = pytest.mark.gpu

FIGS = ("iters", "ok", "bit_err", "pre_err", "erased", "pay_err", "nstat2", "nbeta")
EXTRA = {"stream", "ext", "half_err"}


def _code(case):
    from vae_equalizer_amd.engine import HammingCode, ProductCode
    return ProductCode(HammingCode(*K.CODES[case.col]), HammingCode(*K.CODES[case.row]))


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
    return len(K.CODES[case.col][0]) * len(K.CODES[case.row][0]), case.K1 * case.K2


@pytest.mark.parametrize("case", K.CASES + K.LARGE + K.TINY[-1:], ids=lambda c: c.name)
def test_tpc_matches_model(case):
    llr, bits = K.tensors(case)
    _check(_run(case, llr, bits), K.expected(case), *_sizes(case), case.name)


def test_grid_stride():
    case = K.STRIDE
    llr, bits = K.tensors(case)
    _check(_run(case, llr, bits), K.expected(case), *_sizes(case), case.name)


@pytest.mark.parametrize("case", [K.CASES[i] for i in (2, 7, 9, 12)] + [K.LARGE[0]], ids=lambda c: c.name)
def test_repeatable_and_outputs_optional(case):
    llr, bits = K.tensors(case)
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
    case = next(c for c in K.CASES if c.w == 4 and c.col == "h7")      # three spare symbols behind the C blocks: no further block fits
    llr, bits = K.tensors(case)
    code = _code(case)
    fit = (llr.shape[-1] - case.t0) * case.w // code.n
    assert fit == case.C and (code.col.k, code.row.k) == (4, 11)
    ret = tpc_decode(torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda(), code, t0=case.t0, want_stream=True, want_ext=True, want_profile=True)
    finite = np.where(np.isfinite(llr), np.abs(llr), np.float32(0.0))
    scale = ret["scale"].cpu().numpy()
    print(f"defaults: {fit} blocks, scale {scale.tolist()} against numpy's {finite.reshape(case.R, -1).mean(1, dtype=np.float32).tolist()}")
    assert scale.dtype == np.float32 and np.allclose(scale, finite.reshape(case.R, -1).mean(1, dtype=np.float64), rtol=1e-5)
    assert ret["alpha"] == tuple(float(v) for v in T.schedule(T.ALPHA, 4)) and ret["beta"] == tuple(float(v) for v in T.schedule(T.BETA, 4))
    assert ret["clip"] == 2.0 ** 60
    want = T.decode(llr, bits, *K.cols(case), 4, 4, T.schedule(T.ALPHA, 4), T.schedule(T.BETA, 4), scale, T.CLIP, 4, 11, case.t0, fit)
    _check(ret, want, code.n, 44, "defaults")
    ret = tpc_decode(torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda(), code, t0=case.t0, scale=0.75, iters=1, want_stream=True, want_ext=True,
                     want_profile=True)
    want = T.decode(llr, bits, *K.cols(case), 4, 1, T.schedule(T.ALPHA, 1), T.schedule(T.BETA, 1), np.full(case.R, 0.75, np.float32), T.CLIP, 4, 11,
                    case.t0, fit)
    _check(ret, want, code.n, 44, "scale-as-a-number")


def test_null_scale_is_one():
    """scale == NULL at the C ABI (engine.tpc_decode always passes a tensor): the case's model ran with 1.0."""
    import ctypes as C
    from vae_equalizer_amd import _native as nat
    case = next(c for c in K.CASES if c.scale is None and c.p > 0)
    llr, bits = K.tensors(case)
    code, (alpha, beta) = _code(case), K.schedules(case)
    L, B = torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda()
    out = torch.empty(case.R, case.C, 8, dtype=torch.int32, device="cuda")
    ext = torch.empty(case.R, case.C, code.n, dtype=torch.float32, device="cuda")
    nat.check(nat.lib().vaeq_tpc_decode(case.R, case.C, llr.shape[-1], case.w, case.t0, code.col.n, code.col.r, code.col.cols.ctypes.data_as(C.c_void_p),
                                        code.row.n, code.row.r, code.row.cols.ctypes.data_as(C.c_void_p), nat.ptr(L), nat.ptr(B, torch.int8), case.p,
                                        case.iters, alpha.ctypes.data_as(C.c_void_p), beta.ctypes.data_as(C.c_void_p), None, case.clip, case.K1, case.K2,
                                        nat.ptr(out, torch.int32), None, None, nat.ptr(ext), None, nat.current_stream(L.device)), "vaeq_tpc_decode")
    torch.cuda.synchronize()
    want = K.expected(case)
    assert want[0][..., 7].sum() > 0                           # positions at +-beta: the scale is seen
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(ext.cpu().numpy().view(np.uint32), want[3].view(np.uint32))
