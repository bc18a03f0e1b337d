"""The model of the window decoder (tests/_ref_ldpc_sc.py) before anything on a GPU is compared with it: the ring model and the scalar restatement on
the dense coupled H agree bit for bit; a window that covers the whole chain is _ref_ldpc.decode on the coupled shifts; sc_array_code has no
4-cycles; and the seeded cases of tests/test_ldpc_sc_gpu.py show every behaviour the kernel has to get right, so that no GPU test passes
vacuously.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

import _ref_ldpc as B
import _ref_ldpc_sc as M


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def _chain(comp, Z, Lc, sigma, seed, plant=False):
    n = Lc * comp.shape[2] * Z
    llr, bits = M.make_case(seed, n, sigma, 1, 1, 12, 3, plant=plant)
    return B.codewords(llr, 3, 1, n)[0, 0], B.codewords(bits, 3, 1, n)[0, 0]


HOLES = M.holes_components(5, 1, 2, 6, 13, ((2, 3), (3, 2)))


@pytest.mark.parametrize("comp,Z,Lc,W,iters,T,sigma,plant", [
    (M.array_components(2, 4, 7), 7, 6, 4, 4, None, 0.6, False),
    (M.array_components(2, 4, 7), 7, 6, 3, 3, 1, 0.8, True),
    (M.array_components(2, 4, 7), 7, 5, 7, 5, None, 0.7, False),               # one position
    (M.array_components(2, 4, 7), 7, 1, 3, 3, None, 0.9, False),
    (M.array_components(2, 4, 7), 7, 2, 3, 3, 3, 0.9, False),
    (HOLES, 13, 5, 3, 4, 2, 0.9, False),                                        # (an infinity on a check of two edges ends as inf - inf)
], ids=lambda v: None)
def test_the_two_restatements_agree(comp, Z, Lc, W, iters, T, sigma, plant):
    llr, bits = _chain(comp, Z, Lc, sigma, 40 + Lc + W, plant)
    a = M.decode(comp, Z, Lc, llr, bits, W, iters, 0.75, T)
    b = M.decode_scalar(comp, Z, Lc, llr, bits, W, iters, 0.75, T)
    print(f"out {a[0].tolist()} / {b[0].tolist()}; pos_err {a[2].tolist()}; pos_iters {a[3].tolist()}")
    assert _same(a, b)
    assert a[0][3] > 0 and a[0][0] > 0                                           # there was something to decode
    assert not np.isnan(a[1]).any()


@pytest.mark.parametrize("comp,Z,Lc,sigma", [(M.A, 31, 12, 0.55), (M.A, 31, 5, 0.7), (HOLES, 13, 6, 0.8), (M.A, 31, 1, 0.7)], ids=lambda v: None)
def test_a_single_window_is_the_block_decoder(comp, Z, Lc, sigma):
    ms = comp.shape[0] - 1
    llr, bits = _chain(comp, Z, Lc, sigma, 60 + Lc)
    for W in (Lc + ms, Lc + ms + 3):
        for iters in (1, 8):
            out, post, pos_err, pos_iters = M.decode(comp, Z, Lc, llr, bits, W, iters, 0.75, 1)
            want_out, want_post = B.decode(M.coupled_shifts(comp, Lc), Z, llr, bits, iters, 0.75)
            print(f"W={W} iters={iters}: {out.tolist()} against {want_out.tolist()}")
            assert np.array_equal(out[:5], want_out) and out[5] == out[0] and np.array_equal(post.view(np.int32), want_post.view(np.int32))
            assert pos_iters.tolist() == [out[0]] and pos_err.sum() == out[2]


@pytest.mark.parametrize("ms,nb,Z", [(2, 4, 29), (2, 4, 31), (3, 5, 73), (2, 6, 47)])
def test_sc_array_code_has_no_4_cycles(ms, nb, Z):
    from vae_equalizer_amd.engine import sc_array_code
    code = sc_array_code(ms, nb, Z, ms + 3)
    assert np.array_equal(code.components, M.array_components(ms, nb, Z)) and (code.ms, code.mb, code.nb, code.Z, code.L) == (ms, 1, nb, Z, ms + 3)
    assert code.n == (ms + 3) * nb * Z and code.m == (2 * ms + 3) * Z and abs(code.rate - (1 - (2 * ms + 3) / ((ms + 3) * nb))) < 1e-12
    cp = code.coupled()
    assert np.array_equal(cp.shifts, M.coupled_shifts(code.components, code.L)) and cp.Z == Z
    H = cp.H().astype(np.int64)
    assert H.shape == (code.m, code.n) and Z > (2 * nb - 1) * 2 ** ms
    assert (H.sum(0) == ms + 1).all() and H.sum(1).max() == (ms + 1) * nb and H.sum(1).min() == nb
    G = H.T @ H                                                                   # two columns share at most one check
    np.fill_diagonal(G, 0)
    assert G.max() == 1


def _coverage(results, iters):
    """results: (out, post, pos_err, pos_iters, stats) of decode_batch calls with one `iters`."""
    pi = np.concatenate([r[3].reshape(-1) for r in results])
    ok = np.concatenate([r[0][..., 1].reshape(-1) for r in results])
    partial = any(((pe > 0).any(-1) & (pe == 0).any(-1) & (o[..., 2] > 0)).any() for o, _, pe, _, _ in results)
    return dict(idle=int((pi == 0).sum()), some=int(((pi > 0) & (pi < iters)).sum()), stalled=int((pi == iters).sum()), ok=int(ok.sum()),
                failed=int((ok == 0).sum()), partial=bool(partial), ties=sum(r[4].get("ties", 0) for r in results))


def test_the_gpu_cases_cover_what_they_must():
    grid = [M.grid_expected(Lc, w, t0, level) for Lc, w, t0 in M.GRID for level in range(3)]
    cov = _coverage(grid, M.GRID_ITERS)
    print("grid:", cov)
    assert cov["idle"] and cov["some"] and cov["stalled"] and cov["ok"] and cov["failed"] and cov["partial"]
    ties = M.special_expected("planted")[4]["ties"]            # float32 magnitudes do not tie by chance: the erasures of this case make them
    print("ties in the minimum search of the planted case:", ties)
    assert ties > 0
    for name in sorted(M.SPECIAL):
        out, post, pos_err, pos_iters, stats = M.special_expected(name)
        print(f"{name}: iters {out[..., 0].tolist()} ok {out[..., 1].tolist()} post_err {out[..., 2].tolist()} pre_err {out[..., 3].tolist()} "
              f"iters_max {out[..., 5].tolist()}")
        assert (out[..., 3] > 0).all() and (out[..., 0] > 0).any() and not np.isnan(post).any(), name
    k = M.SPECIAL
    assert M.special_expected("iters-100")[0][..., 5].max() > 10                  # the hundred are used beyond what the grid allows
    assert M.special_expected("iters-1")[0][..., 5].max() == 1
    assert not np.array_equal(M.special_expected("alpha-1")[1], M.special_expected("alpha-0.5")[1])
    assert not all(np.array_equal(M.special_expected(a)[3], M.special_expected(b)[3]) for a, b in (("test-1", "test-ms+1"), ("test-ms+1", "test-W")))
    llr, _ = M.special_case("planted")
    assert np.isposinf(llr).any() and np.isneginf(llr).any() and (np.signbit(llr) & (llr == 0)).any() and (~np.signbit(llr) & (llr == 0)).any()
    holes = k["mb-2-holes"]["comp"]
    assert sorted((holes[0] >= 0).sum(1).tolist()) == [2, 3] and sorted((holes[1] >= 0).sum(1).tolist()) == [2, 3]
    assert (k["row-weight-32"]["comp"] >= 0).sum() == 32
    assert M.positions(2, 12, 14) == 1 and M.positions(2, 12, 3) == 12 and M.positions(2, 1, 3) == 1 and M.positions(2, 2, 3) == 2


@pytest.mark.parametrize("level", range(3))
def test_the_three_noise_levels_do_what_they_are_named_for(level):
    """sc_array_code(2, 4, 31, 12), W = 5, iters = 10: sigma 0.4 leaves many positions idle, 0.55 decodes everything within a few iterations per
    position, 0.7 decodes nothing and stalls at every position."""
    res = [M.grid_expected(12, w, t0, level) for w in (12, 8, 6) for t0 in (0, 7)]
    out = np.concatenate([r[0].reshape(-1, 6) for r in res])
    pi = np.concatenate([r[3].reshape(-1, r[3].shape[-1]) for r in res])
    print(f"sigma {M.SIGMAS[level]}: iters {out[:, 0].tolist()} ok {out[:, 1].tolist()} post_err {out[:, 2].tolist()}; idle positions {int((pi == 0).sum())} "
          f"of {pi.size}, most iterations at a position {int(pi.max())}")
    if level == 0:
        assert (out[:, 1] == 1).all() and (out[:, 2] == 0).all() and (pi == 0).sum() > pi.size // 2 and out[:, 0].max() > 0
    elif level == 1:
        assert (out[:, 1] == 1).all() and (out[:, 2] == 0).all() and pi.max() < M.GRID_ITERS and (out[:, 0] > 0).all()
    else:
        assert (out[:, 1] == 0).all() and (out[:, 2] > 0).all() and (pi == M.GRID_ITERS).all()
