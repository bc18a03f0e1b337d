"""The integer model of the fixed-point window decoder (tests/_ref_ldpc_sc_q.py) before anything on a GPU is compared with it: the ring model and
the scalar restatement agree in every output on every case of tests/test_ldpc_sc_q_gpu.py; a window that covers the whole chain is
_ref_ldpc_q.decode on the coupled shifts; and the seeded cases show every rule of the header binding somewhere, so that no GPU test passes
vacuously.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

import _ref_ldpc as B
import _ref_ldpc_q as Q
import _ref_ldpc_sc as M
import _ref_ldpc_sc_q as S


def _scalar_batch(comp, Z, Lc, llr, bits, t0, C, W, prm, iters, T):
    n = Lc * comp.shape[2] * Z
    lc, bc = B.codewords(llr, t0, C, n), B.codewords(bits, t0, C, n)
    res = [[S.decode_scalar(comp, Z, Lc, lc[r, c], bc[r, c], W, prm, iters, T) for c in range(C)] for r in range(llr.shape[0])]
    return tuple(np.array([[x[k] for x in row] for row in res]) for k in range(4))


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[1].dtype == b[1].dtype == np.int16


@pytest.mark.parametrize("Lc,w,t0", S.GRID)
def test_the_two_restatements_agree_on_the_grid(Lc, w, t0):
    for level in range(3):
        llr, bits = S.grid_case(Lc, w, t0, level)
        a = S.grid_expected(Lc, w, t0, level)
        b = _scalar_batch(S.A, 31, Lc, llr, bits, t0, S.C_, S.GRID_W, S.DEFAULT, S.GRID_ITERS, None)
        print(f"sigma {S.SIGMAS[level]}: iters {a[0][..., 0].tolist()} ok {a[0][..., 1].tolist()} post_err {a[0][..., 2].tolist()}")
        assert _same(a, b)


@pytest.mark.parametrize("name", sorted(S.SPECIAL))
def test_the_two_restatements_agree_on_the_corners(name):
    k = S.SPECIAL[name]
    llr, bits = S.special_case(name)
    a = S.special_expected(name)
    b = _scalar_batch(k["comp"], k["Z"], k["Lc"], llr, bits, k["t0"], k["C"], k["W"], k["prm"], k["iters"], k["T"])
    print(f"{name}: out {a[0].tolist()} / {b[0].tolist()}")
    assert _same(a, b)


@pytest.mark.parametrize("comp,Z,Lc,sigma", [(M.A, 31, 12, 0.55), (M.A, 31, 5, 0.7), (M.holes_components(5, 1, 2, 6, 13, ((2, 3), (3, 2))), 13, 6, 0.8),
                                             (M.A, 31, 1, 0.7)], ids=lambda v: None)
@pytest.mark.parametrize("prm", ["A", "B", "D"])
def test_a_single_window_is_the_fixed_point_block_decoder(comp, Z, Lc, sigma, prm):
    ms, n = comp.shape[0] - 1, Lc * comp.shape[2] * Z
    prm = Q.SETS[prm]
    llr, bits = Q.make_case_q(60 + Lc, n, sigma, 1, 1, 12, 3, prm["scale"])
    llr, bits = B.codewords(llr, 3, 1, n)[0, 0], B.codewords(bits, 3, 1, n)[0, 0]
    for W in (Lc + ms, Lc + ms + 3):
        for iters in (1, 8):
            out, post, pos_err, pos_iters = S.decode(comp, Z, Lc, llr, bits, W, prm, iters, 1)
            want_out, want_post = Q.decode(M.coupled_shifts(comp, Lc), Z, llr, bits, prm, iters, S.new_stats())
            print(f"W={W} iters={iters}: {out.tolist()} against {want_out.tolist()}")
            assert np.array_equal(out[:5], want_out) and out[5] == out[0] and post.dtype == np.int16 and np.array_equal(post, want_post)
            assert pos_iters.tolist() == [out[0]] and pos_err.sum() == out[2] and out[3] > 0 and out[0] > 0


def test_the_gpu_cases_cover_what_they_must():
    results = [S.grid_expected(Lc, w, t0, level) for Lc, w, t0 in S.GRID for level in range(3)] + [S.special_expected(n) for n in sorted(S.SPECIAL)]
    total = {k: sum(r[4][k] for r in results) for k in S.STATS}
    out = np.concatenate([r[0].reshape(-1, 6) for r in results])
    idle, worked, failed = int((out[:, 0] == 0).sum()), int(((out[:, 1] == 1) & (out[:, 0] > 0)).sum()), int((out[:, 1] == 0).sum())
    print(f"{total}; of {len(out)} chains {idle} idle, {worked} decoded after work, {failed} failed")
    for k in ("channel_clamp", "message_clamp", "app_clamp", "f_zero", "tie_not_first", "ring_wraps", "head_rows", "tail_rows", "half", "nan"):
        assert total[k] > 0, k
    assert idle and worked and failed
    assert ((out[:, 1] == 1) & (out[:, 0] > 0) & (out[:, 2] == 0) & (out[:, 3] > 0)).any()       # errors went in and none came out
    long = S.special_expected("long-chain")
    print("long-chain:", long[4], "iterations per position", long[3].ravel().tolist())
    assert long[4]["ring_wraps"] >= 2 and long[4]["head_rows"] > 0 and long[4]["tail_rows"] > 0 and long[3].shape[-1] == 56
    grid = {k: sum(r[4][k] for r in results[:3 * len(S.GRID)]) for k in S.STATS}
    assert grid["head_rows"] > 0 and grid["tail_rows"] > 0 and grid["ring_wraps"] > 0
    era = S.special_expected("scale-1e-30")[0]
    assert (era[..., 4] == 1488).all()                                            # everything is erased
    assert S.special_expected("scale-1e30")[4]["channel_clamp"] > 4 * 1400
    assert S.special_expected("bits-2")[4]["app_clamp"] > 0 and S.special_expected("offset-min-sum")[4]["f_zero"] > 0
    llr, _ = S.special_case("planted-q")
    assert np.isnan(llr).any() and np.isposinf(llr).any() and all((llr == np.float32(v / 0.5)).any() for v in (0.5, -0.5, 1.5, -1.5, 2.5, -2.5))
    llr, _ = S.special_case("planted")
    assert np.isposinf(llr).any() and np.isneginf(llr).any() and (np.signbit(llr) & (llr == 0)).any()
    assert S.DEFAULT == dict(bits=5, scale=2.0 ** 0, app_bits=7, num=6, beta=0)


def test_the_identity_input_clamps_nothing():
    """Small-integer LLRs under IDENTITY (bits 8, app_bits 15, scale 1, f the identity): no clamp of any kind binds and nothing is rounded, so the
    integer decoder computes what float32 min-sum at alpha = 1 computes on the same input -- every value an integer of magnitude below 2^24.  The
    float model agrees with the integer one in every output: the ground of the device-against-device identity in tests/test_ldpc_sc_q_gpu.py."""
    llr, bits = S.identity_case()
    assert np.array_equal(llr, np.rint(llr)) and not np.signbit(llr[llr == 0]).any() and np.abs(llr).max() <= 6
    stats = S.new_stats()
    a = S.decode_batch(S.A, 31, 12, llr, bits, 7, S.C_, S.GRID_W, S.IDENTITY, S.GRID_ITERS, stats=stats)
    b = M.decode_batch(S.A, 31, 12, llr, bits, 7, S.C_, S.GRID_W, S.GRID_ITERS, 1.0)
    print(stats, "iters", a[0][..., 0].tolist(), "ok", a[0][..., 1].tolist(), "pre_err", a[0][..., 3].tolist(), "post_err", a[0][..., 2].tolist())
    assert stats["channel_clamp"] == stats["message_clamp"] == stats["app_clamp"] == stats["half"] == stats["nan"] == 0
    assert (a[0][..., 0] > 0).all() and (a[0][..., 3] > 0).all() and stats["tie_not_first"] > 0 and 0 < a[0][..., 1].sum() < a[0][..., 1].size
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].astype(np.float32), b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
