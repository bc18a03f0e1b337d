"""vaeq_ldpc_sc_decode and vaeq_ldpc_sc_decode_q over the parts of include/vaeq.h's envelope that tests/test_ldpc_sc_gpu.py and
tests/test_ldpc_sc_q_gpu.py leave out, through engine.ldpc_sc_decode(..., want_post=True, want_profile=True) against the models
tests/_ref_ldpc_sc.py and tests/_ref_ldpc_sc_q.py with no tolerance: np.array_equal on the six counters, post (float32 through a uint32 view,
int16 directly), pos_err, pos_iters and the derived BER_post, BER_pre and FER.  The cases live in tests/_ldpc_sc_envelope_cases.py (its docstring
lists them group by group); tests/test_ref_ldpc_sc_envelope_host.py asserts on the CPU that the models reach in them what this file relies on,
and that wrong variants of the models fail them.  Every test prints its figures before it asserts.

  memory 4 .. 7 (d << 23 all ones, row weight 32 with eight components), rows that are head and tail at once, mb = 3 and 4 with unequal rows and
  empty (d, l), nb = 32 at the largest Z of either decoder, W = 32 (the ring of 39 slots), Z at 2, 3 and around 64, 128 and 512 with shifts 0 and
  Z - 1, the ways Lc, W and ms meet, every T, w in {1, 5, 7, 13, 64} in frames with no symbol to spare, the grids 1 x 40, 40 x 1 and 5 x 3, 100
  iterations and 1, the fixed-point kernel's shared address/value register at the largest ring and the widest values, its absent edges in head
  rows whose real edges all sit at Mmax, and planted non-finite inputs.

Then device against device, no model in the loop: a chain decoded alone against the same chain inside a grid, every window that covers the chain
against the smallest such window, a single window against engine.ldpc_decode on code.coupled(), and the float decoder at alpha = 1 on small
integers against the fixed-point one with f the identity."""
import numpy as np
import pytest
import torch

import _ref_ldpc_sc_q as S
import _ldpc_sc_envelope_cases as E

pytestmark = pytest.mark.gpu

KEYS = ("iters", "ok", "bit_err", "pre_err", "erased", "iters_max")
PROFILE = ("pos_err", "pos_iters")


def _cuda(x):
    return x if torch.is_tensor(x) else torch.from_numpy(np.array(x)).cuda()


def _decode(comp, Z, Lc, llr, bits, W, **kw):
    from vae_equalizer_amd.engine import ScLdpcCode, ldpc_sc_decode
    r = ldpc_sc_decode(_cuda(llr), _cuda(bits), ScLdpcCode(comp, Z, Lc), W, want_post=True, want_profile=True, **kw)
    torch.cuda.synchronize()
    return r


def _run(name, fixed, **kw):
    k = E.CASES[name]
    llr, bits = E.inputs(name)
    args = dict(t0=k["t0"], chains=k["C"], iters=k["iters"], test=k["T"])
    args.update(dict(quant=dict(k["prm"])) if fixed else dict(alpha=k["alpha"]))
    args.update(kw)
    return _decode(k["comp"], k["Z"], k["Lc"], llr, bits, args.pop("W", k["W"]), **args)


def _view(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check(r, want, n, tag, prm=None):
    """test_ldpc_sc_gpu._check and test_ldpc_sc_q_gpu._check in one: prm None = the float decoder."""
    want_out, want_post, want_err, want_iters = want[:4]
    got_out = np.stack([r[k].cpu().numpy() for k in KEYS], -1)
    got_post, got_err, got_iters = r["post"].cpu().numpy(), r["pos_err"].cpu().numpy(), r["pos_iters"].cpu().numpy()
    shapes = got_post.shape == want_post.shape and got_err.shape == want_err.shape and got_iters.shape == want_iters.shape
    print(f"{tag}: positions {r['positions']}, iterations per position {np.bincount(want_iters.ravel()).tolist()} ok {int(want_out[..., 1].sum())}/"
          f"{want_out[..., 1].size} pre_err {int(want_out[..., 3].sum())} erased {int(want_out[..., 4].sum())} post_err {int(want_out[..., 2].sum())}; "
          f"counters differ in {int((got_out != want_out).sum())}, post in {int((_view(got_post) != _view(want_post)).sum()) if shapes else 'shape'} of "
          f"{want_post.size}, pos_err in {int((got_err != want_err).sum()) if shapes else 'shape'}, pos_iters in "
          f"{int((got_iters != want_iters).sum()) if shapes else 'shape'}")
    assert shapes and got_out.dtype == np.int64 and got_post.dtype == (np.float32 if prm is None else np.int16) == want_post.dtype
    assert r["positions"] == want_iters.shape[-1] and (r["quant"] == prm if prm is not None else "quant" not in r)
    assert np.array_equal(got_out, want_out)
    assert np.array_equal(_view(got_post), _view(want_post))
    assert np.array_equal(got_err, want_err) and np.array_equal(got_iters, want_iters)
    C = want_out.shape[1]
    assert np.array_equal(r["BER_post"].cpu().numpy(), (want_out[..., 2].sum(1) / np.float32(C * n)).astype(np.float32))
    assert np.array_equal(r["BER_pre"].cpu().numpy(), (want_out[..., 3].sum(1) / np.float32(C * n)).astype(np.float32))
    assert np.array_equal(r["FER"].cpu().numpy(), (want_out[..., 2] > 0).mean(1).astype(np.float32))


def _lds(k, fixed):
    from vae_equalizer_amd import _native as nat
    f = nat.lib().vaeq_ldpc_sc_q_lds_bytes if fixed else nat.lib().vaeq_ldpc_sc_lds_bytes
    return int(f(*E.dims(k), k["Z"], k["W"]))


def _frame_is_tight(k, llr, bits):
    """Not one symbol to spare, and what lies outside the chains is loud, wrong and holds an exact zero."""
    n, N = E.n_chain(k), llr.shape[-1]
    free = E.unused(n, k["C"], k["w"], k["t0"], N)
    assert N == k["t0"] + -(-k["C"] * n // k["w"]) and free.any() and not bits[:, free].any()
    assert ((llr[:, free] == E.LOUD) | (llr[:, free] == 0)).all() and ((llr[:, free] == 0).sum(1) == 1).all()


@pytest.mark.parametrize("name", E.FLOAT)
def test_float_kernel_equals_model(name):
    k = E.CASES[name]
    lds = _lds(k, False)
    assert lds == E.lds_f(*E.dims(k), k["Z"], k["W"]) <= 64 * 1024
    if k["spare"] == 0:
        _frame_is_tight(k, *E.inputs(name))
    _check(_run(name, False), E.expected_f(name), E.n_chain(k), f"{name} float alpha={k['alpha']} ({lds} bytes of LDS)")


@pytest.mark.parametrize("name", E.FIXED)
def test_fixed_point_kernel_equals_model(name):
    k = E.CASES[name]
    lds = _lds(k, True)
    assert lds == E.lds_q(*E.dims(k), k["Z"], k["W"]) <= 64 * 1024
    if k["spare"] == 0:
        _frame_is_tight(k, *E.inputs(name))
    _check(_run(name, True), E.expected_q(name), E.n_chain(k), f"{name} {k['prm']} ({lds} bytes of LDS)", k["prm"])


@pytest.mark.parametrize("fixed", (False, True), ids=("float", "fixed"))
def test_nb_32_one_Z_above_the_largest_is_refused(fixed):
    from vae_equalizer_amd import _native as nat
    Z = E.NB32_Z["q" if fixed else "f"]
    f = nat.lib().vaeq_ldpc_sc_q_lds_bytes if fixed else nat.lib().vaeq_ldpc_sc_lds_bytes
    print(f"(ms, mb, nb, W) = (1, 2, 32, 2): Z = {Z} takes {f(1, 2, 32, Z, 2)} bytes, Z = {Z + 1} takes {f(1, 2, 32, Z + 1, 2)}")
    assert f(1, 2, 32, Z, 2) <= 64 * 1024 < f(1, 2, 32, Z + 1, 2)
    llr, bits = E.frame(1, 5 * 32 * (Z + 1), (0.5,), 1, 12, 0)
    with pytest.raises(nat.VaeqError):
        _decode(E.nb32_components(Z + 1), Z + 1, 5, llr, bits, 2, **(dict(quant=dict(bits=5)) if fixed else {}))


@pytest.mark.parametrize("fixed", (False, True), ids=("float", "fixed"))
def test_a_full_row_of_weight_2_is_refused(fixed):
    """One block per component and row: the full rows have two blocks, the first and the last row block one each -- outside the table rule."""
    from vae_equalizer_amd._native import VaeqError
    comp = np.array([[[3, -1, -1]], [[-1, 5, -1]]], np.int32)
    llr, bits = E.frame(2, 4 * 3 * 7, (0.5,), 1, 12, 0)
    with pytest.raises(VaeqError):
        _decode(comp, 7, 4, llr, bits, 2, **(dict(quant=dict(bits=5)) if fixed else {}))


# ------------------------------------------------------------------ device against device
def _table(name):
    """A case's table, or the nb = 32 table at a Z small enough for wide windows."""
    return (E.nb32_components(8), 8) if name == "nb32-Z8" else (E.CASES[name]["comp"], E.CASES[name]["Z"])


def _windows(comp, Z, fixed, Ws):
    """Those of the windows Ws whose state fits."""
    ms, mb, nb = comp.shape[0] - 1, comp.shape[1], comp.shape[2]
    return [W for W in sorted(set(Ws)) if (E.lds_q if fixed else E.lds_f)(ms, mb, nb, Z, W) <= 64 * 1024]


def _same(a, b, keys=KEYS + PROFILE + ("post",)):
    return {x: int((_view(a[x].cpu().numpy()) != _view(b[x].cpu().numpy())).sum()) if a[x].shape == b[x].shape else "shape" for x in keys}


@pytest.mark.parametrize("fixed", (False, True), ids=("float", "fixed"))
def test_a_chain_alone_is_the_chain_in_the_grid(fixed):
    """Chain c of run r of the 5 x 3 grid (w = 7, t0 = 3, chains that start inside a symbol) in a frame of its own: R = C = 1, t0 = 0."""
    name = "bitmap-R5-C3"
    k = E.CASES[name]
    llr, bits = E.inputs(name)
    big = _run(name, fixed)
    kw = dict(quant=dict(k["prm"])) if fixed else dict(alpha=k["alpha"])
    for r, c in ((0, 0), (1, 2), (2, 1), (4, 2), (3, 0)):
        one = _decode(k["comp"], k["Z"], k["Lc"], *E.lone_chain(k, llr, bits, r, c), k["W"], chains=1, iters=k["iters"], **kw)
        part = {x: big[x][r:r + 1, c:c + 1] for x in KEYS + PROFILE + ("post",)}
        diff = _same(one, part)
        print(f"run {r} chain {c}: iters {int(one['iters'])} ok {int(one['ok'])} pre_err {int(one['pre_err'])} post_err {int(one['bit_err'])}; alone "
              f"and in the grid differ in {diff}")
        assert not any(diff.values())
    assert int(big["iters"].min()) < int(big["iters"].max()) and int(big["pre_err"].min()) > 0


WIDE = [("tables-t4-ms1", 5), ("tables-t4-ms2-reversed", 4), ("tables-t3-ms3", 4), ("memory-ms7-W8", 3), ("nb32-Z8", 3), ("Z-65", 4)]


@pytest.mark.parametrize("fixed", (False, True), ids=("float", "fixed"))
@pytest.mark.parametrize("name,Lc", WIDE)
def test_every_window_that_covers_the_chain_gives_the_same(name, Lc, fixed):
    comp, Z = _table(name)
    ms = comp.shape[0] - 1
    llr, bits = E.frame(700 + Lc, Lc * comp.shape[2] * Z, (0.5, 0.9), 2, 8, 5)
    kw = dict(quant=dict(bits=5)) if fixed else {}
    wider = _windows(comp, Z, fixed, (Lc + ms + 1, (Lc + ms + 32) // 2, 32))
    assert len(wider) >= 2
    for T in (1, Lc + ms):
        a = _decode(comp, Z, Lc, llr, bits, Lc + ms, t0=5, chains=2, iters=6, test=T, **kw)
        for W in wider:
            b = _decode(comp, Z, Lc, llr, bits, W, t0=5, chains=2, iters=6, test=T, **kw)
            diff = _same(a, b)
            print(f"{name} Lc={Lc} T={T} W={Lc + ms} against W={W}: iters {a['iters'].ravel().tolist()} ok {a['ok'].ravel().tolist()} post_err "
                  f"{a['bit_err'].ravel().tolist()}; differ in {diff}")
            assert a["positions"] == b["positions"] == 1 and not any(diff.values())
        assert int(a["iters"].sum()) > 0 and int(a["pre_err"].sum()) > 0


BLOCK = [("tables-t4-ms1", 1), ("tables-t4-ms1-reversed", 1), ("memory-ms7-W8", 1), ("memory-ms4-W5", 4), ("memory-ms5-W6", 2), ("nb32-Z8", 2),
         ("Z-512", 2), ("Z-2", 7)]


@pytest.mark.parametrize("quant", [None, dict(bits=5), dict(bits=4, scale=0.5, app_bits=4, num=8, beta=1)], ids=["float", "5-bit", "4-bit-offset"])
@pytest.mark.parametrize("name,Lc", BLOCK)
def test_one_position_is_the_block_decoder_on_the_device(name, Lc, quant):
    """W >= Lc + ms: the five shared counters and every bit of post are engine.ldpc_decode's on code.coupled(), in float and with quant; the
    chains are short enough for the coupled table to lie inside the block decoder's envelope ((Lc + ms) mb <= 8 block rows, Lc nb <= 64)."""
    from vae_equalizer_amd.engine import ScLdpcCode, ldpc_decode
    comp, Z = _table(name)
    code = ScLdpcCode(comp, Z, Lc)
    assert (Lc + code.ms) * code.mb <= 8 and Lc * code.nb <= 64
    llr, bits = (_cuda(x) for x in E.frame(600 + Lc, code.n, (0.5, 0.9), 3, 8, 5))
    kw = {} if quant is None else dict(quant=quant)
    for W in _windows(comp, Z, quant is not None, (Lc + code.ms, min(Lc + code.ms + 4, 32))):
        for iters in (1, 7):
            a = _decode(comp, Z, Lc, llr, bits, W, t0=5, chains=3, iters=iters, test=1, **kw)
            b = ldpc_decode(llr, bits, code.coupled(), t0=5, codewords=3, max_iter=iters, want_post=True, **kw)
            torch.cuda.synchronize()
            diff = _same(a, b, KEYS[:5] + ("post",))
            print(f"{name} Lc={Lc} W={W} iters={iters}: iters {b['iters'].tolist()} ok {b['ok'].tolist()} post_err {b['bit_err'].tolist()}; the two "
                  f"differ in {diff}")
            assert a["positions"] == 1 and not any(diff.values()) and a["post"].dtype == b["post"].dtype and a.get("quant") == b.get("quant")
            assert torch.equal(a["iters"], a["iters_max"]) and torch.equal(a["pos_iters"][..., 0], a["iters"])
            assert torch.equal(a["pos_err"].sum(-1), a["bit_err"]) and int(b["pre_err"].sum()) > 0 and int(b["iters"].sum()) > 0


@pytest.mark.parametrize("name", sorted(E.IDENTITY_CASES))
def test_the_float_decoder_at_alpha_1_on_small_integers(name):
    """f the identity at bits = 8, app_bits = 15, scale = 1 on small-integer LLRs: no clamp binds (the host file counts none on the model), so the
    float kernel at alpha = 1 computes the same integers -- on an ms = 7 table and on an mb = 4 table, both with empty (d, l)."""
    comp, Z, Lc, W, _ = E.IDENTITY_CASES[name]
    llr, bits = E.identity_inputs(name)
    a = _decode(comp, Z, Lc, llr, bits, W, t0=7, chains=2, iters=10, quant=dict(S.IDENTITY))
    b = _decode(comp, Z, Lc, llr, bits, W, t0=7, chains=2, iters=10, alpha=1.0)
    print(f"{name}: iters {a['iters'].tolist()} / {b['iters'].tolist()} ok {a['ok'].tolist()} pre_err {a['pre_err'].tolist()} post_err "
          f"{a['bit_err'].tolist()}; post differs in {int((a['post'].float() != b['post']).sum())} of {b['post'].numel()}, largest |post| "
          f"{float(b['post'].abs().max())}")
    assert "quant" not in b and a["post"].dtype == torch.int16 and b["post"].dtype == torch.float32
    assert all(torch.equal(a[x], b[x]) for x in KEYS + PROFILE)
    assert torch.equal(a["post"].float(), b["post"]) and int(a["iters"].min()) > 0 and int(a["pre_err"].min()) > 0
