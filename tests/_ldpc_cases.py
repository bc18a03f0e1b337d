"""What the LDPC GPU tests share: the call into engine.ldpc_decode, the comparison with a model's counters and final values that prints its
figures and then asserts np.array_equal (float32 `post` through a uint32 view, int16 `post` directly), and the cases of
tests/test_ldpc_envelope_gpu.py -- the codes, the seeded inputs and the models' answers, built and decoded once.  The host tests
(tests/test_ref_ldpc_host.py, test_ref_ldpc_q_host.py, test_ref_ldpc_il_host.py) assert on the CPU that these cases reach what the GPU test relies on.

_decode, _counters        the call with want_post=True; out[R, C, 5] of its result;
_check, _check_q          the assertions against (want_out, want_post), float32 and int16;
code(), Case, inputs(),   a case is a code name and the shape of its batch; inputs() builds its tensors (contiguous or behind the interleaver,
expected(), run()         for the float or the fixed-point decoder), expected() decodes them with the model, run() holds the device to it;
mixed_shifts() ...        the new tables: row weights that differ from layer to layer, nb = 64, Z at the wave boundary with planted shifts;
saturated(), integers()   inputs with planted infinities; integer LLRs on which float32 min-sum at alpha = 1 is exact;
most_iterations()         the codewords of a case that the host tests hold to the scalar restatements;
deinterleave()            the interleaver's permutation from the header's sentence, without tests/_ref_ldpc_il.py.
"""
import collections
import functools

import numpy as np

import _ref_ldpc as M
import _ref_ldpc_il as IL
import _ref_ldpc_q as Q

F = np.float32


# ------------------------------------------------------------------ the call and the comparison
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _decode(shifts, Z, llr, bits, **kw):
    import torch
    from vae_equalizer_amd.engine import LdpcCode, ldpc_decode
    to = lambda x: x if torch.is_tensor(x) else torch.from_numpy(x).cuda()
    r = ldpc_decode(to(llr), to(bits), LdpcCode(shifts, Z), want_post=True, **kw)
    torch.cuda.synchronize()
    return r


def _counters(r):
    return np.stack([r[k].cpu().numpy() for k in ("iters", "ok", "bit_err", "pre_err", "erased")], -1)


def _figures(r, want_out, n):
    C = want_out.shape[1]
    assert np.array_equal(r["BER_post"].cpu().numpy(), (want_out[..., 2].sum(1) / np.float32(C * n)).astype(np.float32))
    assert np.array_equal(r["BER_pre"].cpu().numpy(), (want_out[..., 3].sum(1) / np.float32(C * n)).astype(np.float32))
    assert np.array_equal(r["FER"].cpu().numpy(), (want_out[..., 2] > 0).mean(1).astype(np.float32))


def _check(r, want_out, want_post, n, tag):
    got_out, got_post = _counters(r), r["post"].cpu().numpy()
    print(f"{tag}: iters {np.bincount(want_out[..., 0].ravel()).tolist()} ok {int(want_out[..., 1].sum())}/{want_out[..., 1].size} "
          f"pre_err {int(want_out[..., 3].sum())} post_err {int(want_out[..., 2].sum())} erased {int(want_out[..., 4].sum())}; "
          f"counters differ in {int((got_out != want_out).sum())}, post in {int((_bits(got_post) != _bits(want_post)).sum())} of {want_post.size}")
    assert got_out.dtype == np.int64 and got_post.dtype == np.float32 and got_post.shape == want_post.shape
    assert np.array_equal(got_out, want_out)
    assert np.array_equal(got_post, want_post) and np.array_equal(_bits(got_post), _bits(want_post))
    _figures(r, want_out, n)


def _check_q(r, want_out, want_post, n, tag):
    got_out, got_post = _counters(r), r["post"].cpu().numpy()
    print(f"{tag}: iters {np.bincount(want_out[..., 0].ravel()).tolist()} ok {int(want_out[..., 1].sum())}/{want_out[..., 1].size} "
          f"pre_err {int(want_out[..., 3].sum())} post_err {int(want_out[..., 2].sum())} erased {int(want_out[..., 4].sum())}; "
          f"counters differ in {int((got_out != want_out).sum())}, post in {int((got_post != want_post).sum())} of {want_post.size}")
    assert got_out.dtype == np.int64 and got_post.dtype == np.int16 and want_post.dtype == np.int16 and got_post.shape == want_post.shape
    assert np.array_equal(got_out, want_out)
    assert np.array_equal(got_post, want_post)
    _figures(r, want_out, n)


# ------------------------------------------------------------------ the new tables
WEIGHTS = (2, 8, 9, 16, 17, 25, 31, 32)                    # both sides of every boundary of the edge walker's groups of eight
MIXED_SEED = 3
Z_FLOAT_64, Z_Q_64 = 186, 315                              # the largest Z at mb = 2, nb = 64: 65 472 bytes of float32 state, 65 520 of fixed-point
Z_WAVE = (63, 64, 65, 511, 512)


def mixed_shifts(seed, weights, nb, Z):
    """Layer l has weights[l] blocks at seeded columns with seeded shifts; drawn again until every column is used by some layer."""
    rng = np.random.default_rng(seed)
    while True:
        s = np.full((len(weights), nb), -1, np.int32)
        for l, wt in enumerate(weights):
            s[l, rng.choice(nb, wt, replace=False)] = rng.integers(0, Z, wt)
        if (s >= 0).any(0).all():
            return s


def nb64_shifts(Z):
    """array_shifts(2, 64, Z) with 32 of its 64 blocks per row kept (a row of 64 is outside the envelope): columns 0 .. 15 and 48 .. 63 in layer
    0, columns 32 .. 63 in layer 1, so that both rows carry the largest column and its last 16 columns lie on both."""
    s = M.array_shifts(2, 64, Z)
    s[0, 16:48] = -1
    s[1, :32] = -1
    return s


def planted_shifts(Z):
    """A seeded irregular 4 x 10 table with two holes per row; the first block of row 0 gets the largest shift Z - 1 (with check Z - 1 the
    largest sum i + s the edge walker folds), the last block of row 3 shift 0."""
    s = M.irregular_shifts(100 + Z, 4, 10, Z, 2)
    s[0, np.nonzero(s[0] >= 0)[0][0]] = Z - 1
    s[3, np.nonzero(s[3] >= 0)[0][-1]] = 0
    return s


@functools.lru_cache(maxsize=None)
def code(name):
    """-> (shifts, Z)."""
    if name in M.CODES:
        return M.CODES[name]
    if name == "mixed":
        return mixed_shifts(MIXED_SEED, WEIGHTS, 40, 65), 65
    if name == "mixed-reversed":
        return np.ascontiguousarray(code("mixed")[0][::-1]), 65
    if name.startswith("nb64-"):
        Z = int(name[5:])
        return nb64_shifts(Z), Z
    if name.startswith("planted-"):
        Z = int(name[8:])
        return planted_shifts(Z), Z
    if name == "smallest":
        return M.array_shifts(1, 2, 2), 2
    raise KeyError(name)


# ------------------------------------------------------------------ cases
Case = collections.namedtuple("Case", "code w t0 R C sigma seed max_iter", defaults=(20,))

# The fixed-point parameter sets of the envelope test, beside _ref_ldpc_q.SETS.
QSETS = dict(Q.SETS)
QSETS.update({
    "num1-beta127": dict(bits=5, scale=1.0, app_bits=7, num=1, beta=127),      # f is 0 everywhere: no message ever moves L
    "8-8": dict(bits=8, scale=8.0, app_bits=8, num=8, beta=0),                 # app_bits == bits: the a-posteriori clamp binds first
    "2-2": dict(bits=2, scale=0.125, app_bits=2, num=6, beta=0),               # every value in {-1, 0, 1}
    "tiny": dict(bits=5, scale=1e-30, app_bits=7, num=6, beta=0),              # every finite input rounds to zero
    "huge": dict(bits=5, scale=1e30, app_bits=7, num=6, beta=0),               # every input that is not zero clips to +-Cmax
    "identity": dict(bits=8, scale=1.0, app_bits=15, num=8, beta=0),           # f(m) = m, no clamp on small integers
})
EXTRA = (-np.inf, 1e-40, -0.0, 0.0)                        # planted as they are, not over the scale: -inf, a subnormal, both zeros


def n_of(case):
    shifts, Z = code(case.code)
    return shifts.shape[1] * Z


def _where(case, depth):
    if depth:
        sym, plane = IL.il_map(case.t0, case.C, n_of(case), case.w, depth)
        return lambda g: (int(plane.ravel()[g]), int(sym.ravel()[g]))
    return lambda g: (g % case.w, case.t0 + g // case.w)


@functools.lru_cache(maxsize=None)
def inputs(case, depth=None, quant=None, extra=False):
    """-> (llr[R,w,N] float32, bits[R,w,N] int8).  depth None: _ref_ldpc.make_case's bit-packed tensors, else _ref_ldpc_il.make_case_il's (not one
    symbol to spare, loud unused planes).  quant (a name in QSETS): _ref_ldpc_q's planted values over the set's scale, through the same map;
    extra: EXTRA planted too, all at distinct codeword bits of every run."""
    n = n_of(case)
    if depth:
        llr, bits = IL.make_case_il(case.seed, n, case.sigma, case.R, case.C, case.w, case.t0, depth)
    else:
        llr, bits = M.make_case(case.seed, n, case.sigma, case.R, case.C, case.w, case.t0)
    if quant is not None:
        llr = llr.copy()
        scale = QSETS[quant]["scale"]
        where, rng = _where(case, depth), np.random.default_rng(case.seed + 7777)
        values = [F(v / scale) for v in Q.PLANTED] + ([F(v) for v in EXTRA] if extra else [])
        for r in range(case.R):
            for g, val in zip(rng.choice(case.C * n, len(values), replace=False), values):
                p, s = where(int(g))
                llr[r, p, s] = val
    return llr, bits


def model(case, llr, bits, depth=None, quant=None, alpha=0.75, max_iter=None, stats=None):
    shifts, Z = code(case.code)
    max_iter = case.max_iter if max_iter is None else max_iter
    with np.errstate(invalid="ignore"):
        if quant is not None:
            return Q.decode_batch(shifts, Z, llr, bits, case.t0, case.C, QSETS[quant], max_iter, depth or 0, stats)
        if depth:
            return IL.decode_batch_il(shifts, Z, llr, bits, case.t0, case.C, depth, max_iter, alpha)
        return M.decode_batch(shifts, Z, llr, bits, case.t0, case.C, max_iter, alpha)


@functools.lru_cache(maxsize=None)
def expected(case, depth=None, quant=None, alpha=0.75, extra=False):
    """-> (out[R,C,5] int64, post[R,C,n]) of the model on inputs(case, depth, quant, extra)."""
    return model(case, *inputs(case, depth, quant, extra), depth, quant, alpha)


def codewords_of(case, x, depth=None):
    n = n_of(case)
    return IL.codewords_il(x, case.t0, case.C, n, depth) if depth else M.codewords(x, case.t0, case.C, n)


def most_iterations(out, k=2):
    """The k codewords (run, codeword) of out[R, C, 5] with the most iterations: the ones the host tests hold to the scalar restatements."""
    C = out.shape[1]
    return [(int(g) // C, int(g) % C) for g in np.argsort(-out[..., 0].ravel(), kind="stable")[:k]]


def run(case, depth=None, quant=None, alpha=None, extra=False, given=None, tag=""):
    """The device against the model on one case; given = (llr, bits, want_out, want_post) replaces inputs() and expected()."""
    shifts, Z = code(case.code)
    llr, bits, want_out, want_post = given or (*inputs(case, depth, quant, extra), *expected(case, depth, quant, 0.75 if alpha is None else alpha, extra))
    kw = dict(t0=case.t0, codewords=case.C, max_iter=case.max_iter, depth=depth)
    kw.update(dict(quant=QSETS[quant]) if quant is not None else dict(alpha=alpha))
    tag = (f"{case.code} w={case.w} t0={case.t0} R={case.R} C={case.C} sigma={case.sigma} max_iter={case.max_iter} depth={depth} "
           f"{'set ' + quant if quant else 'float alpha=' + str(alpha)} {tag}")
    r = _decode(shifts, Z, llr, bits, **kw)
    (_check_q if quant is not None else _check)(r, want_out, want_post, n_of(case), tag)
    return r


# 1. mixed row weights, 2. nb = 64, 3. Z at the wave boundary
MIXED = {(name, sigma): Case(name, 4, 3, 2, 3, sigma, 5, 100) for name in ("mixed", "mixed-reversed") for sigma in (0.25, 0.45)}
NB64 = {(Z, sigma): Case(f"nb64-{Z}", 2, 1, 1, 2, sigma, 900 + int(100 * sigma), 100) for Z in (Z_FLOAT_64, Z_Q_64) for sigma in (0.3, 0.4)}
WAVE = {(Z, sigma): Case(f"planted-{Z}", 2, 1, 2, 3, sigma, 300 + Z + int(100 * sigma)) for Z in Z_WAVE for sigma in (0.55, 0.65)}

# 4. every w
WIDTHS = (1, 2, 3, 4, 5, 7, 13, 64)
W_CODES = ("array-3-6-7", "irregular-5-12-80")


def width_case(name, w, t0, level):
    return Case(name, w, t0, M.R_, M.C_, M.SIGMAS[level], 20000 + 1000 * W_CODES.index(name) + 10 * w + 3 * level + (t0 > 0))


# 5. the grid: many codewords in one run, many runs of one codeword, one workgroup
GRID = {
    "C=300": (Case("smallest", 3, 5, 1, 300, 0.8, 41), (1, 7, 300)),
    "R=40": (Case("array-3-6-7", 12, 5, 40, 1, 0.5, 42), (1,)),
    "one": (Case("array-3-6-7", 12, 5, 1, 1, 0.5, 43), (1,)),
}

# 6. ragged groups of more than one codeword: C = 7 at depth 4 is 4 + 3, at depth 3 is 3 + 3 + 1
RAGGED_C, RAGGED_DEPTHS = 7, (3, 4, 7)
RAGGED = (("array-3-6-7", 4), ("array-3-6-7", 12), ("irregular-5-12-80", 8))


def ragged_case(name, w, level):
    return Case(name, w, 11, M.R_, RAGGED_C, M.SIGMAS[level], 30000 + 100 * w + 10 * level + len(name))


# 7. alpha: 0.7 rounds in almost every product (0.75 and 0.8125 have 2 and 4 mantissa bits), 1.0 and 0.5 in none
ALPHAS = (0.7, 1.0, 0.5)
ALPHA_CASE = Case("irregular-5-12-80", 8, 11, M.R_, M.C_, M.SIGMAS[1], M.case_seed("irregular-5-12-80", 8, 11, 1))

# 8. saturated inputs, 9. the fixed-point parameter corners
SATURATED_CASE = Case("array-4-24-31", 12, 11, M.R_, M.C_, M.SIGMAS[1], 8001)
CORNER_SETS = ("num1-beta127", "8-8", "2-2", "tiny", "huge")


def corner_case(name, level, quant):
    return Case(name, 12, 11, M.R_, M.C_, M.SIGMAS[level], 9000 + 10 * level + len(name), 100 if quant == "num1-beta127" else 20)


@functools.lru_cache(maxsize=None)
def saturated():
    """-> (llr, bits, want_out, want_post, wrong): SATURATED_CASE's tensors with one infinity per codeword that carries the sign of its TX bit,
    and in codeword `wrong` = (run, codeword) a second one of the wrong sign.  Every row of array-4-24-31 has 24 edges and at most two infinite
    ones, so m1 and m2 stay finite and no inf - inf arises."""
    case = SATURATED_CASE
    n = n_of(case)
    llr, bits = (a.copy() for a in inputs(case))
    rng = np.random.default_rng(case.seed + 1)
    where = _where(case, None)
    wrong = (1, 3)
    for r in range(case.R):
        for c in range(case.C):
            j = rng.choice(n, 2, replace=False)
            for k, sign in enumerate((1.0, -1.0) if (r, c) == wrong else (1.0,)):
                p, s = where(c * n + int(j[k]))
                llr[r, p, s] = F(sign * (np.inf if bits[r, p, s] == 0 else -np.inf))
    return (llr, bits, *model(case, llr, bits), wrong)


# C 1. float equals fixed point where nothing clamps
INTEGER_CASE = Case("irregular-5-12-80", 12, 3, 2, 3, 0.0, 1, 30)


@functools.lru_cache(maxsize=None)
def integers():
    """-> (llr[2,12,3+240] float32, bits): magnitudes uniform in 0 .. 6 that carry the sign of the TX bit (a zero of a 1 bit is -0.0), flipped with
    probability 0.02.  n % w == 0, so the tensor is the contiguous form and the interleaved one with not a symbol to spare alike."""
    case = INTEGER_CASE
    rng = np.random.default_rng(case.seed)
    N = case.t0 + case.C * n_of(case) // case.w
    bits = rng.integers(0, 2, (case.R, case.w, N)).astype(np.int8)
    mag = rng.integers(0, 7, bits.shape).astype(F)
    flip = rng.random(bits.shape) < 0.02
    llr = (mag * np.where((bits != 0) ^ flip, F(-1.0), F(1.0))).astype(F)
    return llr, bits


# C 2. interleaved equals contiguous on de-interleaved input
def deinterleave(x, t0, C, S, depth):
    """x[R,w,N] -> the tensor whose symbol t0 + c S + u is x's symbol of codeword c, symbol u under vaeq_ldpc_decode_il's sentence in
    include/vaeq.h: group k = c / depth holds D_k = min((k + 1) depth, C) - k depth codewords from base t0 + k depth S, and the codeword with
    local index d has its symbol u at base + u D_k + d."""
    y = x.copy()
    for c in range(C):
        k = c // depth
        D, d, base = min((k + 1) * depth, C) - k * depth, c - k * depth, t0 + k * depth * S
        for u in range(S):
            y[..., t0 + c * S + u] = x[..., base + u * D + d]
    return y
