"""vaeq_ldpc_sc_decode (the sliding-window decoder of spatially coupled LDPC chains) against the float32 model tests/_ref_ldpc_sc.py, through
engine.ldpc_sc_decode.

No tolerance: the header fixes the decoder down to the order of its individually rounded float32 operations, so out, post, pos_err and pos_iters
have to be the model's; a differing value is a contraction, an ordering bug or a slip in the window's ring.  tests/test_ref_ldpc_sc_host.py pins
the model to an independent restatement and to the block decoder's model, and asserts that the seeded cases below reach idle positions, positions
that take some and all of their iterations, decoded and undecoded chains, chains with errors in some column blocks only, and ties.

Cases (tests/_ref_ldpc_sc.py): the grid -- sc_array_code(2, 4, 31, Lc) with Lc = 12 and 11 (1364 bits: chains start inside a symbol), W = 5 (the
ring of 7 slots wraps), three noise levels, w in {12, 8, 6}, t0 in {0, 7}, R = 3, C = 2 -- and SPECIAL, one named corner each.  The single-window
call is also held to engine.ldpc_decode on code.coupled(), device against device.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import _ref_ldpc_sc as M

pytestmark = pytest.mark.gpu

KEYS = ("iters", "ok", "bit_err", "pre_err", "erased", "iters_max")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _decode(comp, Z, Lc, llr, bits, W, **kw):
    from vae_equalizer_amd.engine import ScLdpcCode, ldpc_sc_decode
    to = lambda x: x if torch.is_tensor(x) else torch.from_numpy(x).cuda()
    kw.setdefault("want_post", True)
    kw.setdefault("want_profile", True)
    r = ldpc_sc_decode(to(llr), to(bits), ScLdpcCode(comp, Z, Lc), W, **kw)
    torch.cuda.synchronize()
    return r


def _counters(r):
    return np.stack([r[k].cpu().numpy() for k in KEYS], -1)


def _check(r, want, n, tag):
    want_out, want_post, want_err, want_iters = want[:4]
    got_out, got_post, got_err, got_iters = _counters(r), r["post"].cpu().numpy(), r["pos_err"].cpu().numpy(), r["pos_iters"].cpu().numpy()
    print(f"{tag}: positions {r['positions']}, iterations per position {np.bincount(want_iters.ravel()).tolist()} ok {int(want_out[..., 1].sum())}/"
          f"{want_out[..., 1].size} pre_err {int(want_out[..., 3].sum())} post_err {int(want_out[..., 2].sum())}; counters differ in "
          f"{int((got_out != want_out).sum())}, post in {int((_bits(got_post) != _bits(want_post)).sum())} of {want_post.size}, pos_err in "
          f"{int((got_err != want_err).sum())}, pos_iters in {int((got_iters != want_iters).sum())}")
    assert got_out.dtype == np.int64 and got_post.dtype == np.float32 and got_post.shape == want_post.shape and r["positions"] == want_iters.shape[-1]
    assert np.array_equal(got_out, want_out)
    assert np.array_equal(_bits(got_post), _bits(want_post))
    assert np.array_equal(got_err, want_err) and np.array_equal(got_iters, want_iters)
    C = want_out.shape[1]
    assert np.array_equal(r["BER_post"].cpu().numpy(), (want_out[..., 2].sum(1) / np.float32(C * n)).astype(np.float32))
    assert np.array_equal(r["BER_pre"].cpu().numpy(), (want_out[..., 3].sum(1) / np.float32(C * n)).astype(np.float32))
    assert np.array_equal(r["FER"].cpu().numpy(), (want_out[..., 2] > 0).mean(1).astype(np.float32))


@pytest.mark.parametrize("Lc,w,t0", M.GRID)
def test_the_grid_against_the_model(Lc, w, t0):
    for level in range(3):
        llr, bits = M.grid_case(Lc, w, t0, level)
        r = _decode(M.A, 31, Lc, llr, bits, M.GRID_W, t0=t0, chains=M.C_, iters=M.GRID_ITERS)
        _check(r, M.grid_expected(Lc, w, t0, level), Lc * 124, f"Lc={Lc} w={w} t0={t0} sigma={M.SIGMAS[level]}")


def _special(name, **kw):
    k = M.SPECIAL[name]
    llr, bits = M.special_case(name)
    return _decode(k["comp"], k["Z"], k["Lc"], llr, bits, k["W"], t0=k["t0"], chains=k["C"], iters=k["iters"], alpha=k["alpha"], test=k["T"], **kw)


@pytest.mark.parametrize("name", sorted(M.SPECIAL))
def test_the_corners_against_the_model(name):
    from vae_equalizer_amd import _native as nat
    k = M.SPECIAL[name]
    ms, mb, nb = k["comp"].shape[0] - 1, k["comp"].shape[1], k["comp"].shape[2]
    lds = nat.lib().vaeq_ldpc_sc_lds_bytes(ms, mb, nb, k["Z"], k["W"])
    assert 0 < lds <= 64 * 1024 and (name != "state-65520" or lds == 65520)
    _check(_special(name), M.special_expected(name), k["Lc"] * nb * k["Z"], f"{name} ({lds} bytes of LDS)")


def test_the_state_just_above_64_KiB_is_refused():
    from vae_equalizer_amd._native import VaeqError
    k = M.SPECIAL["state-65520"]
    llr, bits = M.make_case(1, 4 * 6 * 391, 0.6, 1, 1, 12, 0)
    with pytest.raises(VaeqError):
        _decode(M.array_components(1, 6, 391), 391, 4, llr, bits, k["W"])


@pytest.mark.parametrize("name,Lc", [("one-position", 6), ("one-position", 5), ("Lc-1", 1), ("Lc-ms", 2), ("mb-2-holes", 3), ("Z-65", 4)])
def test_one_position_is_the_block_decoder_on_the_device(name, Lc):
    """W >= Lc + ms: the five shared counters and every bit of post are engine.ldpc_decode's on code.coupled(); no model in the loop.  The chains
    are short enough for the coupled table to lie inside the block decoder's envelope ((Lc + ms) mb <= 8 block rows)."""
    from vae_equalizer_amd.engine import ScLdpcCode, ldpc_decode
    k = M.SPECIAL[name]
    code = ScLdpcCode(k["comp"], k["Z"], Lc)
    assert (Lc + code.ms) * code.mb <= 8
    llr, bits = (torch.from_numpy(x).cuda() for x in M.make_case(600 + Lc, code.n, 0.7, 2, 3, 8, 5))
    for W in (Lc + code.ms, min(Lc + code.ms + 4, 32)):
        for iters in (1, 7):
            a = _decode(k["comp"], k["Z"], Lc, llr, bits, W, t0=5, chains=3, iters=iters, test=1)
            b = ldpc_decode(llr, bits, code.coupled(), t0=5, codewords=3, max_iter=iters, want_post=True)
            torch.cuda.synchronize()
            print(f"{name} Lc={Lc} W={W} iters={iters}: iters {b['iters'].tolist()} ok {b['ok'].tolist()} post_err {b['bit_err'].tolist()}; the two "
                  f"differ in {sum(int((a[x] != b[x]).sum()) for x in KEYS[:5])} counters")
            assert a["positions"] == 1 and all(torch.equal(a[x], b[x]) for x in KEYS[:5]) and torch.equal(a["iters"], a["iters_max"])
            assert torch.equal(a["post"].view(torch.int32), b["post"].view(torch.int32)) and int(b["pre_err"].sum()) > 0 and int(b["iters"].sum()) > 0
            assert torch.equal(a["pos_iters"][..., 0], a["iters"]) and torch.equal(a["pos_err"].sum(-1), a["bit_err"])


def test_the_optional_outputs_change_nothing_and_two_calls_agree():
    a = _special("planted")
    for post, profile in ((False, False), (True, False), (False, True)):
        b = _special("planted", want_post=post, want_profile=profile)
        assert ("post" in b) == post and ("pos_err" in b) == profile and ("pos_iters" in b) == profile
        assert np.array_equal(_counters(a), _counters(b)) and all(torch.equal(a[x], b[x]) for x in ("BER_post", "BER_pre", "FER"))
    b = _special("planted")
    assert np.array_equal(_counters(a), _counters(b)) and torch.equal(a["post"].view(torch.int32), b["post"].view(torch.int32))
    assert torch.equal(a["pos_err"], b["pos_err"]) and torch.equal(a["pos_iters"], b["pos_iters"])


def test_default_chains_test_and_refusals():
    from vae_equalizer_amd._native import VaeqError
    from vae_equalizer_amd.engine import LdpcCode
    llr, bits = M.grid_case(12, 12, 0, 1)                                         # 251 symbols of 12 bits: two chains of 1488 bits and 3 symbols over
    r = _decode(M.A, 31, 12, llr, bits, M.GRID_W)
    _check(r, M.grid_expected(12, 12, 0, 1), 1488, "defaults: chains = the most that fit, iters = 10, test = ms + 1")
    assert tuple(_decode(M.A, 31, 12, llr, bits, M.GRID_W, t0=4)["iters"].shape) == (3, 1)   # 2964 bits left: one chain
    with pytest.raises(ValueError):
        _decode(M.A, 31, 12, llr, bits, M.GRID_W, t0=200)                          # 612 bits left: none
    with pytest.raises(VaeqError):
        _decode(M.A, 31, 12, llr, bits, M.GRID_W, chains=3)
    with pytest.raises(VaeqError):
        _decode(M.A, 31, 12, llr, bits, 2)                                        # a window of ms row blocks
    from vae_equalizer_amd.engine import ldpc_sc_decode
    with pytest.raises(ValueError):
        ldpc_sc_decode(torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda(), LdpcCode(M.coupled_shifts(M.A, 3), 31), 5)


def test_outer_is_bch_outer_on_the_column_blocks():
    """outer= on a decodable case: bch_outer by hand over post seen as [R, C L, nb Z], the default payload (nb - mb) Z of every column block."""
    from vae_equalizer_amd.engine import BchCode, ScLdpcCode, bch_outer, ldpc_sc_decode
    llr, bits = (torch.from_numpy(x).cuda() for x in M.grid_case(12, 8, 7, 1))
    code, bch = ScLdpcCode(M.A, 31, 12), BchCode(7, 2)
    kw = dict(t0=7, chains=M.C_, iters=1)                                         # one iteration per position: errors are left for the outer code
    a = ldpc_sc_decode(llr, bits, code, M.GRID_W, outer=dict(code=bch), **kw)
    b = ldpc_sc_decode(llr, bits, code, M.GRID_W, want_post=True, **kw)
    want = bch_outer(b["post"].view(M.R_, M.C_ * 12, 124), bits, bch, 124, t0=7, payload=93)
    torch.cuda.synchronize()
    print(f"inner post_err {b['bit_err'].tolist()}; outer status {want['status'].tolist()} pre_err {want['pre_err'].tolist()} post_err {want['bit_err'].tolist()}")
    assert "post" not in a and set(a) == set(b) - {"post"} | {"outer"} and set(a["outer"]) == set(want)
    assert all(torch.equal(a["outer"][x], want[x]) for x in want) and all(torch.equal(a[x], b[x]) for x in KEYS)
    assert int(want["pre_err"].sum()) > 0 and tuple(want["status"].shape) == (M.R_, M.C_ * 12 * 93 // 127)
    with pytest.raises(ValueError):
        ldpc_sc_decode(llr, bits, code, M.GRID_W, outer=dict(code=bch, payload=125), **kw)
