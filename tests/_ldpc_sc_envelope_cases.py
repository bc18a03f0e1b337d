"""The cases of tests/test_ldpc_sc_envelope_gpu.py and tests/test_ref_ldpc_sc_envelope_host.py: what vaeq_ldpc_sc_decode and vaeq_ldpc_sc_decode_q
(include/vaeq.h) accept and the cases of their feature commits (tests/_ref_ldpc_sc.py, tests/_ref_ldpc_sc_q.py) leave out.  No new model: every
case is built here and decoded by those two models, once per process (inputs(), expected_f(), expected_q()).

A case is a dict(group, comp, Z, Lc, W, T, iters, alpha, prm, sigmas, C, w, t0, spare, erasures, plant, kinds, inputs): one run per entry of `sigmas`
(a quiet run and a noisy one, so that a case has chains that decode and chains that fail), kinds "fq" = both decoders, "f" / "q" = one.
frame() makes the tensors: everything outside the chains -- the t0 leading symbols, the spare symbols, the unused planes of a last symbol -- holds
a loud wrong value (-1e4 against a 0 bit) and one exact zero, so a read outside the chains changes pre_err or erased; spare = 0 leaves N not one
symbol to spare.

Groups, by the items of the issue (CASES[name]["group"]):
  memory    array_components(ms, nb, Z) for ms = 4 .. 7 (ms = 7, nb = 4: row weight 32, d << 23 all ones) at W = ms + 1 and W = ms + 5, Lc long
            enough for the column ring of the wider window to wrap three times;
  headtail  Lc < ms, Lc = ms, Lc = ms + 1 at ms = 7 and ms = 4: rows whose head and tail masks bind together, at W = ms + 1 and at W = Lc + ms;
  tables    mb = 4, 4 and 3 with holes, full-row weights 4, 8, 9, 16 / 17, 25, 31, 16 / 32, 9, 8, two (d, l) without any block, each table also
            with its rows l reversed.  A full row of weight 2 does not exist: row block 0 has the blocks of component 0 alone and the last row
            block those of component ms alone, and each needs two, so 4 is the least (the host file asserts this and the GPU file the refusal);
            truncated rows of weight 2 are there;
  nb32      ms = 1, mb = 2, nb = 32, 32 blocks per full row, at the largest Z of either decoder (120 in float, 204 in fixed point);
  window32  W = 32 at ms = 7 (a ring of 39 slots, Lc = 120) and at ms = 1;
  Z         Z in {2, 3, 63, 64, 65, 127, 128, 129, 511, 512} with shifts 0 and Z - 1 in both components;
  meet      Lc + ms = W, Lc + ms = W + 1, Lc < W with P > 1, Lc = W, Lc = W + 1;
  T         every T in 1 .. W on one case.  min(p + T, rows) cannot bind before the last position: p <= P - 2 = rows - W - 1 there, so
            p + T <= rows - 1 (the host file walks the whole envelope for this);
  bitmap    w in {1, 5, 7, 13, 64} at nb Z = 33, t0 = 3, N with no symbol to spare; the grids 1 x 40, 40 x 1 and 5 x 3;
  iters     100 iterations on a chain that never passes, 1 on a decodable one;
  q         fixed point only: the state-65472 shape and a head-row case at bits = 8, app_bits = 15; app_bits = 9 where the a-posteriori clamp
            binds at both signs and |t| goes beyond Lmax; bits = app_bits = 2; num = 1, beta = 127; an input of nothing but +-Mmax, whose first
            layer update is a head row with every real a_e = Mmax; NaN, both infinities, a subnormal and both zeros planted.
            With app_bits = 15 no L reaches +-16383: without a clamp L = channel + the sum of the messages of its checks, at most
            127 (1 + (ms + 1) mb) <= 4191 (asserted in the host file), so Lmax + Mmax is reached at app_bits = 9 instead;
  f         float only: alpha = 0.5 and 1.0 on an ms = 5 case, and both infinities and a -0.0 planted (no NaN: outside the header's contract).
"""
import functools

import numpy as np

import _ref_ldpc as B
import _ref_ldpc_sc as M
import _ref_ldpc_sc_q as S

F = np.float32
LOUD = F(-1e4)
Q_PLANTED = (np.nan, np.inf, -np.inf, 1e-40, 0.0, -0.0)        # 1e-40 is a float32 subnormal


def lds_f(ms, mb, nb, Z, W):
    """vaeq_ldpc_sc_lds_bytes restated: L float32 and the TX bits as bytes per ring entry, four dwords per check of the window."""
    ring = (W + ms) * nb * Z
    return 4 * ring + ((ring + 3) & ~3) + 16 * W * mb * Z


def lds_q(ms, mb, nb, Z, W):
    """vaeq_ldpc_sc_q_lds_bytes restated: L int16 and the TX bits as bytes per ring entry, two dwords per check of the window."""
    ring = (W + ms) * nb * Z
    return ((2 * ring + 3) & ~3) + ((ring + 3) & ~3) + 8 * W * mb * Z


def frame(seed, n, sigmas, C, w, t0, spare=3, erasures=4):
    """llr[R, w, N] float32, bits[R, w, N] int8 with R = len(sigmas), N = t0 + ceil(C n / w) + spare: _ref_ldpc.make_case's recipe at noise
    sigmas[r] in run r, `erasures` exact +0.0 per run inside the chains; outside them LOUD against a 0 bit and, per run, one exact zero."""
    R = len(sigmas)
    rng = np.random.default_rng(seed)
    N = t0 + -(-C * n // w) + spare
    bits = rng.integers(0, 2, (R, w, N)).astype(np.int8)
    sg = np.asarray(sigmas, np.float64)[:, None, None]
    y = (1.0 - 2.0 * bits) + sg * rng.standard_normal((R, w, N))
    llr = (2.0 * y / sg ** 2).astype(F)
    for r in range(R):
        g = rng.choice(C * n, erasures, replace=False)
        llr[r, g % w, t0 + g // w] = F(0.0)
    inside = unused(n, C, w, t0, N) == 0
    llr[:, ~inside], bits[:, ~inside] = LOUD, 0
    free = np.argwhere(~inside)
    if len(free):
        llr[:, free[-1][0], free[-1][1]] = F(0.0)
    return llr, bits


def unused(n, C, w, t0, N):
    """[w, N] bool: the entries that belong to no chain."""
    g = np.arange(N * w).reshape(N, w).T - t0 * w
    return (g < 0) | (g >= C * n)


def plant(llr, seed, values, n_total, w, t0):
    """Per run, the values at len(values) distinct bits inside the chains."""
    rng = np.random.default_rng(seed)
    for r in range(llr.shape[0]):
        g = rng.choice(n_total, len(values), replace=False)
        with np.errstate(all="ignore"):
            llr[r, g % w, t0 + g // w] = np.array(values, np.float64).astype(F)
    return llr


def _case(group, comp, Z, Lc, W, sigmas=(0.45, 0.8), C=2, w=12, t0=5, T=None, iters=10, alpha=0.75, prm=S.DEFAULT, spare=3, erasures=4, plant=None,
          kinds="fq", inputs=None):
    comp = np.array(comp, np.int32)                            # a copy: the caller's table stays writable
    comp.setflags(write=False)
    return dict(group=group, comp=comp, Z=Z, Lc=Lc, W=W, sigmas=tuple(sigmas), C=C, w=w, t0=t0, T=T, iters=iters, alpha=alpha, prm=dict(prm),
                spare=spare, erasures=erasures, plant=plant, kinds=kinds, inputs=inputs)


def dims(k):
    """-> (ms, mb, nb)."""
    return k["comp"].shape[0] - 1, k["comp"].shape[1], k["comp"].shape[2]


# ---- the tables of the group `tables`: keep[d][l] blocks of component d in row l (seeded columns and shifts, _ref_ldpc_sc.holes_components)
TABLES = {
    "t4-ms1": (11, 1, 4, 16, 7, ((2, 3, 4, 8), (2, 5, 5, 8))),                                     # full rows of 4, 8, 9, 16
    "t4-ms2": (12, 2, 4, 12, 5, ((6, 9, 10, 8), (5, 8, 11, 0), (6, 8, 10, 8))),                    # 17, 25, 31, 16; (d, l) = (1, 3) is empty
    "t3-ms3": (13, 3, 3, 8, 9, ((8, 2, 2), (8, 0, 2), (8, 5, 2), (8, 2, 2))),                      # 32, 9, 8; (1, 1) is empty
}
TABLE_WEIGHTS = {"t4-ms1": (4, 8, 9, 16), "t4-ms2": (17, 25, 31, 16), "t3-ms3": (32, 9, 8)}


def table(name, reverse=False):
    seed, ms, mb, nb, Z, keep = TABLES[name]
    comp = M.holes_components(seed, ms, mb, nb, Z, keep)
    return (comp[:, ::-1] if reverse else comp), Z


def nb32_components(Z):
    """ms = 1, mb = 2, nb = 32: row 0 has component 0 in columns 0 .. 15 and component 1 in 16 .. 31, row 1 the other way round; 32 blocks per
    full row, 16 per truncated one, every column block in two checks."""
    c = np.arange(32)
    comp = np.full((2, 2, 32), -1, np.int32)
    comp[0, 0, :16], comp[1, 0, 16:] = (3 * c[:16] + 1) % Z, (5 * c[16:] + 2) % Z
    comp[0, 1, 16:], comp[1, 1, :16] = (7 * c[16:] + 3) % Z, (11 * c[:16] + 4) % Z
    return comp


def z_components(Z):
    """ms = 1, mb = 1, nb = 3 with the shifts 0 and Z - 1 in both components (i + s reaches 2 Z - 2)."""
    return np.array([[[0, Z - 1, 1 % Z]], [[Z - 1, 0, Z // 2]]], np.int32)


NB32_Z = {"f": 120, "q": 204}                                  # the largest Z of (ms, mb, nb, W) = (1, 2, 32, 2); the host file asserts it
Q8 = dict(bits=8, scale=8.0, app_bits=15, num=6, beta=0)
Z_EDGES = (2, 3, 63, 64, 65, 127, 128, 129, 511, 512)
WIDE = 4                                                       # the wider window of `memory` is W = ms + 1 + WIDE

CASES = {}
for _ms, _nb in ((4, 5), (5, 5), (6, 4), (7, 4)):
    for _W in (_ms + 1, _ms + 1 + WIDE):
        CASES[f"memory-ms{_ms}-W{_W}"] = _case("memory", M.array_components(_ms, _nb, 31), 31, 3 * (2 * _ms + 1 + WIDE) + 2, _W,
                                               sigmas=(0.35, 0.5, 0.8), C=1)
for _ms, _Lcs in ((7, (1, 2, 3, 7, 8)), (4, (2, 4, 5))):
    for _Lc in _Lcs:
        for _W in sorted({_ms + 1, _Lc + _ms}):
            CASES[f"headtail-ms{_ms}-Lc{_Lc}-W{_W}"] = _case("headtail", M.array_components(_ms, 4, 13), 13, _Lc, _W, sigmas=(0.6, 1.0))
for _name in TABLES:
    for _rev in (False, True):
        _comp, _Z = table(_name, _rev)
        CASES[f"tables-{_name}{'-reversed' if _rev else ''}"] = _case("tables", _comp, _Z, 9, _comp.shape[0] + 1, sigmas=(0.5, 0.7, 1.0), w=8)
CASES["nb32-Z120"] = _case("nb32", nb32_components(120), 120, 5, 2, sigmas=(0.25, 0.5), C=1)
CASES["nb32-Z204"] = _case("nb32", nb32_components(204), 204, 5, 2, sigmas=(0.25, 0.5), C=1, kinds="q")
CASES["window32-ms7"] = _case("window32", M.array_components(7, 3, 5), 5, 120, 32, sigmas=(0.5, 0.7), C=1, iters=5)
CASES["window32-ms1"] = _case("window32", M.array_components(1, 4, 7), 7, 100, 32, sigmas=(0.45, 0.6), C=1, iters=5)
for _Z in Z_EDGES:
    CASES[f"Z-{_Z}"] = _case("Z", z_components(_Z), _Z, 4, 2, sigmas=(0.45, 0.9), C=2 if _Z < 500 else 1)
for _name, _ms, _Lc, _W in (("P1", 2, 3, 5), ("P2", 2, 4, 5), ("Lc-below-W", 4, 5, 6), ("Lc-W", 2, 5, 5), ("Lc-W+1", 2, 6, 5)):
    CASES[f"meet-{_name}"] = _case("meet", M.array_components(_ms, 3, 13), 13, _Lc, _W, sigmas=(0.6, 1.0))
for _T in range(1, 7):
    CASES[f"T-{_T}"] = _case("T", M.A, 31, 10, 6, T=_T, sigmas=(0.55, 0.62), C=1, inputs="T-1")
for _w in (1, 5, 7, 13, 64):
    CASES[f"bitmap-w{_w}"] = _case("bitmap", M.array_components(1, 3, 11), 11, 5, 3, sigmas=(0.6, 1.0), C=3, w=_w, t0=3, spare=0)
CASES["bitmap-R1-C40"] = _case("bitmap", M.array_components(1, 3, 11), 11, 5, 3, sigmas=(0.8,), C=40, w=7, t0=3, spare=0)
CASES["bitmap-R40-C1"] = _case("bitmap", M.array_components(1, 3, 11), 11, 5, 3, sigmas=(0.6, 0.8, 1.0, 1.2) * 10, C=1, w=7, t0=3, spare=0)
CASES["bitmap-R5-C3"] = _case("bitmap", M.array_components(1, 3, 11), 11, 5, 3, sigmas=(0.6, 0.8, 1.0, 1.2, 0.7), C=3, w=7, t0=3, spare=0)
CASES["iters-100"] = _case("iters", M.array_components(4, 4, 13), 13, 6, 5, sigmas=(0.95,), C=2, iters=100)
CASES["iters-1"] = _case("iters", M.array_components(4, 4, 13), 13, 6, 5, sigmas=(0.6,), C=2, iters=1)
CASES["q-state-65472-app15"] = _case("q", M.array_components(1, 9, 496), 496, 4, 3, sigmas=(0.6,), C=1, prm=dict(Q8, scale=1e30, num=8), kinds="q")
CASES["q-head-rows-app15"] = _case("q", M.array_components(4, 4, 13), 13, 6, 5, sigmas=(0.6, 1.0), prm=Q8, kinds="q")
CASES["q-app9"] = _case("q", M.array_components(4, 4, 13), 13, 6, 5, sigmas=(0.6, 1.0), C=3, prm=dict(Q8, app_bits=9, scale=1e30, num=8), kinds="q")
CASES["q-bits2"] = _case("q", M.array_components(4, 4, 13), 13, 6, 5, sigmas=(0.6, 1.0), prm=dict(bits=2, scale=0.125, app_bits=2, num=6, beta=0),
                         kinds="q")
CASES["q-messages-zero"] = _case("q", M.array_components(4, 4, 13), 13, 6, 5, sigmas=(0.6, 1.0), prm=dict(S.DEFAULT, num=1, beta=127), kinds="q")
for _name, _comp, _Z in (("array-ms4", M.array_components(4, 4, 13), 13), ("t3-ms3", *table("t3-ms3"))):
    CASES[f"q-all-Mmax-{_name}"] = _case("q", _comp, _Z, 6, _comp.shape[0], sigmas=(0.8, 1.2), erasures=0,
                                         prm=dict(bits=2, scale=1e30, app_bits=2, num=8, beta=0), kinds="q")
    CASES[f"q-all-Mmax-{_name}-5bit"] = _case("q", _comp, _Z, 6, _comp.shape[0], sigmas=(0.8, 1.2), erasures=0, prm=dict(S.DEFAULT, scale=1e30), kinds="q")
CASES["q-planted"] = _case("q", M.array_components(4, 4, 13), 13, 6, 5, sigmas=(0.6, 1.0), plant="q", kinds="q")
CASES["f-alpha-0.5"] = _case("f", M.array_components(5, 5, 31), 31, 12, 7, sigmas=(0.5, 0.8), alpha=0.5, kinds="f")
CASES["f-alpha-1.0"] = _case("f", M.array_components(5, 5, 31), 31, 12, 7, sigmas=(0.5, 0.8), alpha=1.0, kinds="f")
CASES["f-planted"] = _case("f", M.array_components(5, 5, 31), 31, 12, 7, sigmas=(0.5, 0.8), plant="inf", kinds="f")

NAMES = sorted(CASES)
FLOAT = [n for n in NAMES if "f" in CASES[n]["kinds"]]
FIXED = [n for n in NAMES if "q" in CASES[n]["kinds"]]


def group(g):
    return [n for n in NAMES if CASES[n]["group"] == g]


def n_chain(k):
    return k["Lc"] * k["comp"].shape[2] * k["Z"]


def _freeze(xs):
    for x in xs:
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return xs


@functools.lru_cache(maxsize=None)
def inputs(name):
    k = CASES[name]
    if k["inputs"] not in (None, name):                             # the tensors of another case: only the decoder's arguments differ
        return inputs(k["inputs"])
    n, seed = n_chain(k), 31000 + 10 * NAMES.index(name)
    llr, bits = frame(seed, n, k["sigmas"], k["C"], k["w"], k["t0"], k["spare"], k["erasures"])
    if k["plant"] == "inf":
        llr = plant(llr, seed + 77, (np.inf, -np.inf, -0.0), k["C"] * n, k["w"], k["t0"])
    elif k["plant"] == "q":
        llr = plant(llr, seed + 77, Q_PLANTED, k["C"] * n, k["w"], k["t0"])
    return _freeze((llr, bits))


@functools.lru_cache(maxsize=None)
def expected_f(name):
    """-> _ref_ldpc_sc.decode_batch's (out, post, pos_err, pos_iters) and the stats dict."""
    k = CASES[name]
    llr, bits = inputs(name)
    stats = {}
    with np.errstate(invalid="ignore"):                        # the planted infinities: inf - inf in a value no output keeps
        return _freeze(M.decode_batch(k["comp"], k["Z"], k["Lc"], llr, bits, k["t0"], k["C"], k["W"], k["iters"], k["alpha"], k["T"], stats)) + (stats,)


@functools.lru_cache(maxsize=None)
def expected_q(name):
    """-> _ref_ldpc_sc_q.decode_batch's (out, post, pos_err, pos_iters) and the stats dict."""
    k = CASES[name]
    llr, bits = inputs(name)
    stats = S.new_stats()
    return _freeze(S.decode_batch(k["comp"], k["Z"], k["Lc"], llr, bits, k["t0"], k["C"], k["W"], k["prm"], k["iters"], k["T"], stats)) + (stats,)


# ---- the device-against-device identities of the GPU file; the host file asserts on the models what they rest on
def sparse_ms7_components():
    """ms = 7, mb = 1, nb = 4 with blocks at offsets 0, 3, 5 and 7 only: row weight 8, every column block in two checks, so that float32 min-sum
    at alpha = 1 stays small (array_components(7, 4, Z) has column weight 8 and outgrows Mmax = 127 within two iterations)."""
    comp, rng = np.full((8, 1, 4), -1, np.int32), np.random.default_rng(5)
    for d, cols in ((0, (0, 1)), (7, (2, 3)), (3, (0, 2)), (5, (1, 3))):
        comp[d, 0, list(cols)] = rng.integers(0, 31, 2)
    return comp


IDENTITY_CASES = {"ms7": (sparse_ms7_components(), 31, 12, 9, 3), "mb4": (table("t4-ms2")[0], 5, 9, 4, 2)}     # comp, Z, Lc, W, the LLRs' amplitude


@functools.lru_cache(maxsize=None)
def identity_inputs(name):
    comp, Z, Lc, _, amp = IDENTITY_CASES[name]
    return _freeze(S.small_integer_case(33000, Lc * comp.shape[2] * Z, 2, 2, 8, 7, sigma=0.45, amp=amp))


def lone_chain(k, llr, bits, r, c):
    """Chain c of run r of a case's tensors, alone in a frame of its own: R = C = 1, t0 = 0, no symbol to spare, LOUD behind the chain."""
    n, w = n_chain(k), k["w"]
    N = -(-n // w)
    out = []
    for x, fill in ((llr, LOUD), (bits, 0)):
        flat = np.full(N * w, fill, x.dtype)
        flat[:n] = B.codewords(x, k["t0"], k["C"], n)[r, c]
        out.append(np.ascontiguousarray(flat.reshape(N, w).T[None]))
    return tuple(out)
