"""vaeq_ldpc_sc_decode_q (the fixed-point sliding-window decoder of spatially coupled LDPC chains) against the integer model
tests/_ref_ldpc_sc_q.py, through engine.ldpc_sc_decode(quant=...).

No tolerance: behind the quantiser every value is an integer and the header fixes every rounding, clamp and tie, so out, post, pos_err and
pos_iters have to be the model's.  tests/test_ref_ldpc_sc_q_host.py pins the model to an independent restatement and to the block decoder's integer
model, and asserts that the seeded cases below make every rule bind: channel, message and a-posteriori clamps, f rounding a message to zero, ties
behind the first edge, ring wraps, head and tail rows with absent edges, idle, decoded and failed chains.

Cases (tests/_ref_ldpc_sc_q.py): the float window tests' grid -- sc_array_code(2, 4, 31, Lc) with Lc = 12 and 11, W = 5, three noise levels, w in
{12, 8, 6}, t0 in {0, 7}, R = 3, C = 2 -- at the 5-bit defaults, and SPECIAL: the float tests' corners at the 5-bit defaults and one corner per rule
of the quantiser.  Two identities hold device against device with no model in the loop: a single window is engine.ldpc_decode(quant=...) on
code.coupled(), and the float window decoder at alpha = 1 on small-integer LLRs is this one with f the identity.  Every test prints its figures
before it asserts."""
import numpy as np
import pytest
import torch

import _ref_ldpc_sc as M
import _ref_ldpc_sc_q as S

pytestmark = pytest.mark.gpu

KEYS = ("iters", "ok", "bit_err", "pre_err", "erased", "iters_max")


def _decode(comp, Z, Lc, llr, bits, W, **kw):
    from vae_equalizer_amd.engine import ScLdpcCode, ldpc_sc_decode
    to = lambda x: x if torch.is_tensor(x) else torch.from_numpy(x).cuda()
    kw.setdefault("want_post", True)
    kw.setdefault("want_profile", True)
    kw.setdefault("quant", dict(bits=5))
    r = ldpc_sc_decode(to(llr), to(bits), ScLdpcCode(comp, Z, Lc), W, **kw)
    torch.cuda.synchronize()
    return r


def _counters(r):
    return np.stack([r[k].cpu().numpy() for k in KEYS], -1)


def _check(r, want, n, prm, tag):
    want_out, want_post, want_err, want_iters = want[:4]
    got_out, got_post, got_err, got_iters = _counters(r), r["post"].cpu().numpy(), r["pos_err"].cpu().numpy(), r["pos_iters"].cpu().numpy()
    print(f"{tag}: positions {r['positions']}, iterations per position {np.bincount(want_iters.ravel()).tolist()} ok {int(want_out[..., 1].sum())}/"
          f"{want_out[..., 1].size} pre_err {int(want_out[..., 3].sum())} erased {int(want_out[..., 4].sum())} post_err {int(want_out[..., 2].sum())}; "
          f"counters differ in {int((got_out != want_out).sum())}, post in {int((got_post != want_post).sum())} of {want_post.size}, pos_err in "
          f"{int((got_err != want_err).sum())}, pos_iters in {int((got_iters != want_iters).sum())}")
    assert got_out.dtype == np.int64 and got_post.dtype == np.int16 and got_post.shape == want_post.shape and r["positions"] == want_iters.shape[-1]
    assert r["quant"] == prm
    assert np.array_equal(got_out, want_out)
    assert np.array_equal(got_post, want_post)
    assert np.array_equal(got_err, want_err) and np.array_equal(got_iters, want_iters)
    C = want_out.shape[1]
    assert np.array_equal(r["BER_post"].cpu().numpy(), (want_out[..., 2].sum(1) / np.float32(C * n)).astype(np.float32))
    assert np.array_equal(r["BER_pre"].cpu().numpy(), (want_out[..., 3].sum(1) / np.float32(C * n)).astype(np.float32))
    assert np.array_equal(r["FER"].cpu().numpy(), (want_out[..., 2] > 0).mean(1).astype(np.float32))


@pytest.mark.parametrize("Lc,w,t0", S.GRID)
def test_the_grid_against_the_model(Lc, w, t0):
    for level in range(3):
        llr, bits = S.grid_case(Lc, w, t0, level)
        r = _decode(S.A, 31, Lc, llr, bits, S.GRID_W, t0=t0, chains=S.C_, iters=S.GRID_ITERS)
        _check(r, S.grid_expected(Lc, w, t0, level), Lc * 124, S.DEFAULT, f"Lc={Lc} w={w} t0={t0} sigma={S.SIGMAS[level]}")


def _special(name, **kw):
    k = S.SPECIAL[name]
    llr, bits = S.special_case(name)
    return _decode(k["comp"], k["Z"], k["Lc"], llr, bits, k["W"], t0=k["t0"], chains=k["C"], iters=k["iters"], test=k["T"], quant=dict(k["prm"]), **kw)


@pytest.mark.parametrize("name", sorted(S.SPECIAL))
def test_the_corners_against_the_model(name):
    from vae_equalizer_amd import _native as nat
    k = S.SPECIAL[name]
    ms, mb, nb = k["comp"].shape[0] - 1, k["comp"].shape[1], k["comp"].shape[2]
    lds = nat.lib().vaeq_ldpc_sc_q_lds_bytes(ms, mb, nb, k["Z"], k["W"])
    assert 0 < lds <= 64 * 1024 and (name != "state-65472" or lds == 65472)
    _check(_special(name), S.special_expected(name), k["Lc"] * nb * k["Z"], k["prm"], f"{name} ({lds} bytes of LDS, {k['prm']})")


def test_the_state_just_above_64_KiB_is_refused():
    from vae_equalizer_amd._native import VaeqError
    llr, bits = M.make_case(1, 4 * 9 * 497, 0.6, 1, 1, 12, 0)
    with pytest.raises(VaeqError):
        _decode(M.array_components(1, 9, 497), 497, 4, llr, bits, 3)


@pytest.mark.parametrize("name,Lc", [("one-position", 6), ("one-position", 5), ("Lc-1", 1), ("Lc-ms", 2), ("mb-2-holes", 3), ("Z-65", 4)])
@pytest.mark.parametrize("quant", [dict(bits=5), dict(bits=4, scale=0.5, app_bits=4, num=8, beta=1)], ids=["5-bit", "4-bit-offset"])
def test_one_position_is_the_fixed_point_block_decoder_on_the_device(name, Lc, quant):
    """W >= Lc + ms: the five shared counters and every bit of the int16 post are engine.ldpc_decode(quant=...)'s on code.coupled(); no model in
    the loop.  The chains are short enough for the coupled table to lie inside the block decoder's envelope ((Lc + ms) mb <= 8 block rows)."""
    from vae_equalizer_amd.engine import ScLdpcCode, ldpc_decode
    k = S.SPECIAL[name]
    code = ScLdpcCode(k["comp"], k["Z"], Lc)
    assert (Lc + code.ms) * code.mb <= 8
    llr, bits = (torch.from_numpy(x).cuda() for x in M.make_case(600 + Lc, code.n, 0.7, 2, 3, 8, 5))
    for W in (Lc + code.ms, min(Lc + code.ms + 4, 32)):
        for iters in (1, 7):
            a = _decode(k["comp"], k["Z"], Lc, llr, bits, W, t0=5, chains=3, iters=iters, test=1, quant=quant)
            b = ldpc_decode(llr, bits, code.coupled(), t0=5, codewords=3, max_iter=iters, want_post=True, quant=quant)
            torch.cuda.synchronize()
            print(f"{name} Lc={Lc} W={W} iters={iters}: iters {b['iters'].tolist()} ok {b['ok'].tolist()} post_err {b['bit_err'].tolist()} erased "
                  f"{b['erased'].tolist()}; the two differ in {sum(int((a[x] != b[x]).sum()) for x in KEYS[:5])} counters")
            assert a["positions"] == 1 and all(torch.equal(a[x], b[x]) for x in KEYS[:5]) and torch.equal(a["iters"], a["iters_max"])
            assert a["post"].dtype == b["post"].dtype == torch.int16 and torch.equal(a["post"], b["post"]) and a["quant"] == b["quant"]
            assert int(b["pre_err"].sum()) > 0 and int(b["iters"].sum()) > 0
            assert torch.equal(a["pos_iters"][..., 0], a["iters"]) and torch.equal(a["pos_err"].sum(-1), a["bit_err"])


def test_the_float_window_decoder_at_alpha_1_on_small_integers():
    """f the identity (num = 8, beta = 0) at bits = 8, app_bits = 15, scale = 1 on LLRs that are small integers: no clamp binds
    (tests/test_ref_ldpc_sc_q_host.py counts none on the model) and nothing is rounded, so the float window kernel at alpha = 1 computes the same
    integers.  Device against device: the six counters, pos_err, pos_iters, and post value for value."""
    llr, bits = (torch.from_numpy(x).cuda() for x in S.identity_case())
    a = _decode(S.A, 31, 12, llr, bits, S.GRID_W, t0=7, chains=S.C_, iters=S.GRID_ITERS, quant=dict(S.IDENTITY))
    b = _decode(S.A, 31, 12, llr, bits, S.GRID_W, t0=7, chains=S.C_, iters=S.GRID_ITERS, quant=None, alpha=1.0)
    print(f"iters {a['iters'].tolist()} / {b['iters'].tolist()} ok {a['ok'].tolist()} pre_err {a['pre_err'].tolist()} post_err {a['bit_err'].tolist()}; "
          f"post differs in {int((a['post'].float() != b['post']).sum())} of {b['post'].numel()}, largest |post| {float(b['post'].abs().max())}")
    assert "quant" not in b and a["post"].dtype == torch.int16 and b["post"].dtype == torch.float32
    assert all(torch.equal(a[x], b[x]) for x in KEYS + ("pos_err", "pos_iters"))
    assert torch.equal(a["post"].float(), b["post"]) and int(a["iters"].min()) > 0 and int(a["pre_err"].min()) > 0


def test_the_optional_outputs_change_nothing_and_two_calls_agree():
    a = _special("planted-q")
    for post, profile in ((False, False), (True, False), (False, True)):
        b = _special("planted-q", want_post=post, want_profile=profile)
        assert ("post" in b) == post and ("pos_err" in b) == profile and ("pos_iters" in b) == profile
        assert np.array_equal(_counters(a), _counters(b)) and all(torch.equal(a[x], b[x]) for x in ("BER_post", "BER_pre", "FER"))
    b = _special("planted-q")
    assert np.array_equal(_counters(a), _counters(b)) and torch.equal(a["post"], b["post"])
    assert torch.equal(a["pos_err"], b["pos_err"]) and torch.equal(a["pos_iters"], b["pos_iters"])


def test_quant_defaults_and_refusals():
    from vae_equalizer_amd._native import VaeqError
    llr, bits = S.grid_case(12, 12, 0, 1)                                         # 251 symbols of 12 bits: two chains of 1488 bits and 3 symbols over
    r = _decode(S.A, 31, 12, llr, bits, S.GRID_W)
    _check(r, S.grid_expected(12, 12, 0, 1), 1488, S.DEFAULT, "defaults: chains = the most that fit, iters = 10, test = ms + 1, quant = dict(bits=5)")
    for bad in (dict(bits=5, width=3), dict(scale=1.0), dict(bits=5.5), 5):
        with pytest.raises(ValueError):
            _decode(S.A, 31, 12, llr, bits, S.GRID_W, quant=bad)
    with pytest.raises(ValueError):                                               # alpha belongs to the float decoder
        _decode(S.A, 31, 12, llr, bits, S.GRID_W, alpha=0.75)
    for bad in (dict(bits=9), dict(bits=1), dict(bits=5, app_bits=4), dict(bits=5, app_bits=16), dict(bits=5, scale=0.0), dict(bits=5, num=9),
                dict(bits=5, beta=128)):
        with pytest.raises(VaeqError):
            _decode(S.A, 31, 12, llr, bits, S.GRID_W, quant=bad)


def test_outer_is_bch_outer_on_the_int16_column_blocks():
    """outer= with quant=: bch_outer by hand over the int16 post seen as [R, C L, nb Z], the default payload (nb - mb) Z of every column block."""
    from vae_equalizer_amd.engine import BchCode, ScLdpcCode, bch_outer, ldpc_sc_decode
    llr, bits = (torch.from_numpy(x).cuda() for x in S.grid_case(12, 8, 7, 1))
    code, bch = ScLdpcCode(S.A, 31, 12), BchCode(7, 2)
    kw = dict(t0=7, chains=S.C_, iters=1, quant=dict(bits=5))                     # one iteration per position: errors are left for the outer code
    a = ldpc_sc_decode(llr, bits, code, S.GRID_W, outer=dict(code=bch), **kw)
    b = ldpc_sc_decode(llr, bits, code, S.GRID_W, want_post=True, **kw)
    assert b["post"].dtype == torch.int16
    want = bch_outer(b["post"].view(S.R_, S.C_ * 12, 124), bits, bch, 124, t0=7, payload=93)
    torch.cuda.synchronize()
    print(f"inner post_err {b['bit_err'].tolist()}; outer status {want['status'].tolist()} pre_err {want['pre_err'].tolist()} post_err {want['bit_err'].tolist()}")
    assert "post" not in a and set(a) == set(b) - {"post"} | {"outer"} and set(a["outer"]) == set(want)
    assert all(torch.equal(a["outer"][x], want[x]) for x in want) and all(torch.equal(a[x], b[x]) for x in KEYS)
    assert int(want["pre_err"].sum()) > 0 and tuple(want["status"].shape) == (S.R_, S.C_ * 12 * 93 // 127)
