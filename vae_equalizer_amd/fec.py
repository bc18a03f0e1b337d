"""The FEC host layer: the code classes, the decoders behind the per-bit LLRs (include/vaeq.h) and the batch runners' fec= dict.  No decoder
has an encoder: each works towards the TX bits and returns counts per codeword, with the rates formed from them on the device."""
import ctypes as C
import math
import numbers

import numpy as np
import torch

from . import _native as nat


def _is_int(x):                                            # an integer of any kind, numpy's included, but no bool
    return isinstance(x, numbers.Integral) and not isinstance(x, bool)


def label_bits(data, n_lev):
    """The transmitted label bits in the plane order of dp_epilogue_llr / awgn_llr: data[..., 2, N] (the TX reference, axis 0 = I, 1 = Q) ->
    int8[..., 2b, N], plane a b + k = bit k of the Gray label t ^ (t >> 1) of the level t = clamp(rint((n-1)/2 data + (n-1)/2), 0, n-1) of
    axis a.  Plain torch ops, on the device data lives on."""
    n = int(n_lev)
    b = n.bit_length() - 1
    scale = 0.5 * (n - 1)
    t = torch.clamp(torch.round(scale * data.to(torch.float16).to(torch.float32) + scale), 0, n - 1).to(torch.int32)
    g = t ^ (t >> 1)
    k = torch.arange(b, dtype=torch.int32, device=data.device)
    bits = (g.unsqueeze(-2) >> k.unsqueeze(-1)) & 1                              # [..., 2, b, N]
    return bits.reshape(*data.shape[:-2], 2 * b, data.shape[-1]).to(torch.int8)


class LdpcCode:
    """A quasi-cyclic LDPC code for ldpc_decode: shifts[mb, nb] of circulant shifts, -1 = a zero block, 0 <= s < Z = the Z x Z block that connects
    check l Z + i to variable c Z + (i + s) mod Z.  n = nb Z bits, m = mb Z checks.  The decoder's envelope (1 <= mb <= 8, 2 <= nb <= 64,
    2 <= Z <= 512, 2 .. 32 non-zero blocks in every block row, 64 KiB of state) is vaeq_ldpc_decode's to refuse."""

    def __init__(self, shifts, Z):
        self.shifts = np.ascontiguousarray(np.asarray(shifts, dtype=np.int32))
        if self.shifts.ndim != 2:
            raise ValueError(f"expected shifts[mb, nb], got shape {self.shifts.shape}")
        self.Z = int(Z)
        self.mb, self.nb = (int(d) for d in self.shifts.shape)
        self.n, self.m = self.nb * self.Z, self.mb * self.Z

    def H(self):
        """The dense parity-check matrix, uint8 [m, n] (for tests: n m bytes)."""
        H = np.zeros((self.m, self.n), np.uint8)
        i = np.arange(self.Z)
        for l in range(self.mb):
            for c in range(self.nb):
                s = int(self.shifts[l, c])
                if s >= 0:
                    H[l * self.Z + i, c * self.Z + (i + s) % self.Z] = 1
        return H


def array_code(mb, nb, Z):
    """The array code: shift (l c) mod Z in block (l, c).  For a prime Z >= nb it has no 4-cycles."""
    return LdpcCode(np.outer(np.arange(mb), np.arange(nb)) % Z, Z)


QUANT_KEYS = ("bits", "scale", "app_bits", "num", "beta")
OUTER_KEYS = ("code", "payload", "spread", "codewords")
OUTER_POST_BYTES = 256 << 20                               # fec_figures with an outer code: the most bytes of `post` alive at a time


def resolve_quant(quant):
    """ldpc_decode's quant= dict(bits, scale=None, app_bits=None, num=6, beta=0) with its defaults filled in: app_bits = bits + 2 and
    scale = 2 ** (bits - 5), a clip near +-16 nats at every width and one nat per step at 5 bits.  ValueError for an unknown key, a missing or
    non-integer bits; the ranges are vaeq_ldpc_decode_q's to refuse."""
    if not isinstance(quant, dict) or set(quant) - set(QUANT_KEYS) or "bits" not in quant:
        raise ValueError(f"quant takes a dict of {', '.join(QUANT_KEYS)} with bits in it; got {sorted(quant) if isinstance(quant, dict) else quant!r}")
    bits = quant["bits"]
    if not _is_int(bits):
        raise ValueError(f"quant['bits'] is an integer number of bits, got {bits!r}")
    bits = int(bits)
    scale, app = quant.get("scale"), quant.get("app_bits")
    return dict(bits=bits, scale=2.0 ** (bits - 5) if scale is None else float(scale), app_bits=bits + 2 if app is None else int(app),
                num=int(quant.get("num", 6)), beta=int(quant.get("beta", 0)))


def _fit(N, w, n, t0, depth):
    """The most codewords of n bits that fit behind t0 into N symbols of w bits: bit-packed (depth None) or in whole symbols."""
    if depth is None:
        return (N - int(t0)) * w // n if n > 0 else 0
    return (N - int(t0)) // -(-n // w) if n > 0 and w > 0 else 0


def _ldpc_rule(alpha, quant):
    """alpha= and quant= of ldpc_decode and ldpc_sc_decode -> (alpha with its default, the resolved quant dict or None)."""
    if quant is not None:
        if alpha is not None:
            raise ValueError("alpha belongs to the float decoder; the fixed-point one is normalised by quant['num'] and quant['beta']")
        quant = resolve_quant(quant)
    return (0.75 if alpha is None else alpha), quant


def _frame(llr, bits):
    """What every decoder takes: llr and bits of one shape [R,2,2b,N] or [R,w,N] -> (dev, R, N, w, llr[R,w,N], bits[R,w,N]), both contiguous."""
    if llr.shape != bits.shape or llr.dim() not in (3, 4):
        raise ValueError(f"expected llr and bits of one shape [R,2,2b,N] or [R,w,N], got {tuple(llr.shape)}, {tuple(bits.shape)}")
    R, N = llr.shape[0], llr.shape[-1]
    llr = llr.reshape(R, -1, N).contiguous()
    return llr.device, R, N, llr.shape[1], llr, bits.reshape(R, -1, N).contiguous()


def _count(given, what, N, w, n, t0, depth):
    """The codewords (chains, blocks: `what`) of a run: as given, or the most that fit behind t0, which must be one at least."""
    if given is not None:
        return int(given)
    C_ = _fit(N, w, n, t0, depth)
    if C_ < 1:
        raise ValueError(f"no {what} of {n} bits fits into {N - int(t0)} symbols of {w} bits")
    return C_


def _payload(K, n, refusal, whole=False):
    """K, the first bits of a codeword of n that are payload: 1 .. n (n None: no upper end), an integer already if `whole` -> int(K)."""
    if (whole and not _is_int(K)) or int(K) < 1 or (n is not None and int(K) > n):
        raise ValueError(refusal)
    return int(K)


def _share(counts, total):
    """counts[R, C] (int64 or bool) -> float32[R]: a run's sum as a share of `total`, in float64 and rounded once.  The divisor is a tensor of
    max(total, 1): a true division, not the product with 1 / total that a Python number would get."""
    tot = torch.full((counts.shape[0],), float(max(total, 1)), dtype=torch.float64, device=counts.device)
    return (counts.sum(1).double() / tot).float()


def _figures(out, C_, n, P=None):
    """The columns the LDPC, staircase and product decoders share: out[R, C, >= 5] int32 -> (out as int64, dict); P: a window decoder's positions."""
    o = out.long()
    ret = dict(iters=o[..., 0], ok=o[..., 1], bit_err=o[..., 2], pre_err=o[..., 3], erased=o[..., 4],
               BER_post=_share(o[..., 2], C_ * n), BER_pre=_share(o[..., 3], C_ * n), FER=_share(o[..., 2] > 0, C_))
    if P is not None:
        ret.update(iters_max=o[..., 5], positions=P)
    return o, ret


def _status_figures(o):
    """The columns bch_outer and chase_decode share, from out[R, C, >= 4] as int64: what became of each word, and the two ways to err unseen."""
    return dict(status=o[..., 0], pre_err=o[..., 1], bit_err=o[..., 2], nflip=o[..., 3],
                miscorrected=((o[..., 0] == 1) & (o[..., 2] > 0)).sum(1), undetected=((o[..., 0] == 0) & (o[..., 1] > 0)).sum(1))


def _stream(want, R, length, dev):
    """The tensors of a want_stream's stream = dict(llr[R,1,length] f32, bits[R,1,length] int8), or (None, None)."""
    return tuple(torch.empty(R, 1, length, dtype=t, device=dev) if want else None for t in (torch.float32, torch.int8))


def ldpc_decode(llr, bits, code, t0=0, codewords=None, max_iter=20, alpha=None, want_post=False, depth=None, quant=None, outer=None):
    """Post-FEC figures of per-bit LLRs on the device (vaeq_ldpc_decode): layered normalized min-sum towards the syndrome of the TX bits (no
    encoder).  llr f32 and bits int8 of one shape, [R,2,2b,N] (dp_epilogue_llr / cma_epilogue_llr with label_bits) or [R,w,N] (awgn_llr,
    awgn_track_llr); bit j of codeword c of a run is global bit c n + j, at symbol t0 + (c n + j) // w in plane (c n + j) % w.  codewords: per
    run, default the most that fit behind t0.  -> dict(iters, ok, bit_err, pre_err, erased [R,C] int64; BER_post[R], BER_pre[R], FER[R] f32
    (FER: the share of codewords with bit_err > 0); post[R,C,n] f32, the final LLRs in codeword order, if want_post).  alpha defaults to 0.75.
    depth: an int puts a symbol interleaver over groups of `depth` codewords in front of the decoder (vaeq_ldpc_decode_il): codewords of
    S = ceil(n / w) whole symbols, symbol u of the codeword with local index d of a group of D at symbol base + u D + d; codewords then defaults
    to (N - t0) // S.  None: the contiguous bit-packed codewords above.
    quant: dict(bits, scale=None, app_bits=None, num=6, beta=0) decodes in fixed point instead (vaeq_ldpc_decode_q): LLRs quantised to `bits`
    bits as rint(llr * scale) (default scale 2 ** (bits - 5)), `bits`-bit check messages, a-posteriori values saturating at app_bits (default
    bits + 2) bits, messages normalised as max(((num m + 4) >> 3) - beta, 0).  Unlike the float decoder this one sees the scale of the LLRs: what
    a wrong noise variance costs after FEC.  alpha has no meaning there and is a ValueError if passed.  The same dict comes back, post int16,
    erased counting what the quantiser rounded to zero, and the resolved dict under "quant".
    outer: dict(code=BchCode, payload=None, spread=True, codewords=None) puts a hard-decision outer decoder behind this one: bch_outer on the
    final LLRs (kept on the device, returned only with want_post), its dict under "outer".  payload defaults to (nb - mb) Z, the first bits of
    every codeword."""
    if outer is not None:
        outer = resolve_outer(outer, code)
    alpha, quant = _ldpc_rule(alpha, quant)
    dev, R, N, w, llr, bits = _frame(llr, bits)
    n = code.n
    C_ = _count(codewords, "codeword", N, w, n, t0, depth)
    out = torch.empty(R, max(C_, 0), 5, dtype=torch.int32, device=dev)
    post = torch.empty(R, max(C_, 0), n, dtype=torch.float32 if quant is None else torch.int16, device=dev) if want_post or outer is not None else None
    with torch.cuda.device(dev):
        head = (code.mb, code.nb, code.Z, code.shifts.ctypes.data_as(C.c_void_p), nat.ptr(llr), nat.ptr(bits, torch.int8))
        tail = (int(max_iter), nat.ptr(out, torch.int32), nat.ptr(post, torch.float32 if quant is None else torch.int16), nat.current_stream(dev))
        if quant is not None:
            nat.check(nat.lib().vaeq_ldpc_decode_q(R, C_, N, w, int(t0), 0 if depth is None else int(depth), *head, quant["bits"], quant["app_bits"],
                                                   quant["scale"], quant["num"], quant["beta"], *tail), "vaeq_ldpc_decode_q")
        elif depth is None:
            nat.check(nat.lib().vaeq_ldpc_decode(R, C_, N, w, int(t0), *head, float(alpha), *tail), "vaeq_ldpc_decode")
        else:
            nat.check(nat.lib().vaeq_ldpc_decode_il(R, C_, N, w, int(t0), int(depth), *head, float(alpha), *tail), "vaeq_ldpc_decode_il")
    _, ret = _figures(out, C_, n)
    if want_post:
        ret["post"] = post
    if quant is not None:
        ret["quant"] = quant
    if outer is not None:
        ret["outer"] = bch_outer(post, bits, outer["code"], n, t0=t0, depth=depth, payload=outer["payload"], spread=outer["spread"],
                                 codewords=outer["codewords"])
    return ret


class ScLdpcCode:
    """A spatially coupled LDPC code for ldpc_sc_decode: components[ms + 1, mb, nb] of circulant shifts (-1 = a zero block, 0 <= s < Z as in
    LdpcCode) coupled into a terminated chain of L positions.  Block row (t, l), t = 0 .. L + ms - 1, holds components[t - i, l, c] in block
    column (i, c) for 0 <= t - i <= ms.  .ms, .mb, .nb, .Z, .L; .n = L nb Z bits (n_chain), .m = (L + ms) mb Z checks, .rate = the design rate
    1 - (L + ms) mb / (L nb).  The decoder's envelope is vaeq_ldpc_sc_decode's to refuse."""

    def __init__(self, components, Z, L):
        self.components = np.ascontiguousarray(np.asarray(components, dtype=np.int32))
        if self.components.ndim != 3 or self.components.shape[0] < 1:
            raise ValueError(f"expected components[ms + 1, mb, nb], got shape {self.components.shape}")
        self.Z, self.L = int(Z), int(L)
        if self.L < 1:
            raise ValueError(f"a chain has at least one position, got L={L}")
        self.ms = int(self.components.shape[0]) - 1
        self.mb, self.nb = (int(d) for d in self.components.shape[1:])
        self.n, self.m = self.L * self.nb * self.Z, (self.L + self.ms) * self.mb * self.Z
        self.rate = 1.0 - (self.L + self.ms) * self.mb / (self.L * self.nb)

    def coupled(self):
        """The LdpcCode of the coupled shifts[(L + ms) mb, L nb] (for tests and small chains)."""
        s = np.full(((self.L + self.ms) * self.mb, self.L * self.nb), -1, np.int32)
        for i in range(self.L):
            for d in range(self.ms + 1):
                s[(i + d) * self.mb:(i + d + 1) * self.mb, i * self.nb:(i + 1) * self.nb] = self.components[d]
        return LdpcCode(s, self.Z)


def sc_array_code(ms, nb, Z, L):
    """The coupled array code: mb = 1, shift (2^d (2c + 1)) mod Z in component d, column c; column weight ms + 1, row weight (ms + 1) nb.
    For a prime Z > (2 nb - 1) 2^ms the coupled matrix has no 4-cycles.  Why: write b = 2c + 1, odd and at most 2 nb - 1.  A 4-cycle joins two
    row blocks t > t' and two block columns, b at offsets d, d' and b' at offsets e, e' with d - d' = e - e' = t - t' = k, and needs
    b (2^d - 2^d') = b' (2^e - 2^e') mod Z, that is b 2^d' (2^k - 1) = b' 2^e' (2^k - 1).  0 < 2^k - 1 < Z is invertible modulo the prime Z,
    so b 2^d' = b' 2^e' mod Z; both sides are integers below Z, so they are equal as integers, and an odd number times a power of two factors
    in one way: b = b' and d' = e', the same block column twice.  tests/test_ref_ldpc_sc_host.py checks H^T H."""
    d, c = np.arange(int(ms) + 1)[:, None, None], np.arange(int(nb))[None, None, :]
    return ScLdpcCode((2 ** d * (2 * c + 1)) % int(Z), Z, L)


def ldpc_sc_decode(llr, bits, code, window, t0=0, chains=None, iters=10, alpha=None, test=None, want_post=False, want_profile=False, outer=None,
                   quant=None):
    """Post-FEC figures of per-bit LLRs under a spatially coupled code on the device (vaeq_ldpc_sc_decode): a window of `window` row-block
    positions slides along the chain of the ScLdpcCode `code`; at each of the P = max(1, L + ms - window + 1) positions at most `iters`
    iterations of ldpc_decode's layered normalized min-sum over the rows inside, until the rows of the first `test` positions of the window
    (default ms + 1: the rows that touch the block about to leave) are satisfied.  llr, bits, t0 and the bit map as for ldpc_decode with
    n = code.n; chains: per run, default the most that fit behind t0.  alpha defaults to 0.75.
    -> ldpc_decode's dict, a chain where it has a codeword (iters [R,C]: the sum over the positions; ok: every position's last test passed; FER:
    the share of chains with bit_err > 0), plus iters_max [R,C] (the most iterations at one position) and positions (P).  want_post:
    post[R,C,n] f32.  want_profile: pos_err [R,C,L] (the errors of each column block in its final state) and pos_iters [R,C,P].
    outer: as for ldpc_decode, bch_outer over the final LLRs seen as [R, C L, nb Z]: every column block is a codeword of nb Z bits under the
    same bit map, its first (nb - mb) Z bits the default payload.  No interleaver here.
    quant: ldpc_decode's dict(bits, scale=None, app_bits=None, num=6, beta=0) with its defaults decodes in fixed point instead
    (vaeq_ldpc_sc_decode_q): the same window with ldpc_decode's integer layer rule, which sees the scale of the LLRs.  alpha is a ValueError
    then; post is int16, erased counts what the quantiser rounded to zero, and the resolved dict comes back under "quant"."""
    if not isinstance(code, ScLdpcCode):
        raise ValueError(f"ldpc_sc_decode takes an ScLdpcCode, got {code!r}")
    if outer is not None:
        outer = resolve_outer(outer, code)
    alpha, quant = _ldpc_rule(alpha, quant)
    test = code.ms + 1 if test is None else test
    dev, R, N, w, llr, bits = _frame(llr, bits)
    n = code.n
    C_ = _count(chains, "chain", N, w, n, t0, None)
    P = max(1, code.L + code.ms - int(window) + 1)
    Cn = max(C_, 0)
    out = torch.empty(R, Cn, 6, dtype=torch.int32, device=dev)
    post_t = torch.float32 if quant is None else torch.int16
    post = torch.empty(R, Cn, n, dtype=post_t, device=dev) if want_post or outer is not None else None
    pos_err = torch.empty(R, Cn, code.L, dtype=torch.int32, device=dev) if want_profile else None
    pos_iters = torch.empty(R, Cn, P, dtype=torch.int32, device=dev) if want_profile else None
    with torch.cuda.device(dev):
        head = (R, C_, N, w, int(t0), code.ms, code.mb, code.nb, code.Z, code.L, code.components.ctypes.data_as(C.c_void_p), nat.ptr(llr),
                nat.ptr(bits, torch.int8), int(window), int(test))
        tail = (int(iters), nat.ptr(out, torch.int32), nat.ptr(post, post_t), nat.ptr(pos_err, torch.int32), nat.ptr(pos_iters, torch.int32),
                nat.current_stream(dev))
        if quant is not None:
            nat.check(nat.lib().vaeq_ldpc_sc_decode_q(*head, quant["bits"], quant["app_bits"], quant["scale"], quant["num"], quant["beta"], *tail),
                      "vaeq_ldpc_sc_decode_q")
        else:
            nat.check(nat.lib().vaeq_ldpc_sc_decode(*head, float(alpha), *tail), "vaeq_ldpc_sc_decode")
    _, ret = _figures(out, C_, n, P)
    if want_post:
        ret["post"] = post
    if want_profile:
        ret["pos_err"], ret["pos_iters"] = pos_err.long(), pos_iters.long()
    if quant is not None:
        ret["quant"] = quant
    if outer is not None:
        ret["outer"] = bch_outer(post.view(R, Cn * code.L, code.nb * code.Z), bits, outer["code"], code.nb * code.Z, t0=t0, payload=outer["payload"],
                                 spread=outer["spread"], codewords=outer["codewords"])
    return ret


class BchCode:
    """A narrow-sense primitive binary BCH code over GF(2^m) with designed correction t, shortened to n bits (default 2^m - 1), for bch_outer:
    .m, .t, .n, .parity (the size of the union of the cyclotomic cosets of 1 .. 2t modulo 2^m - 1), .k = n - parity, .rate = k / n.  ValueError
    outside vaeq_bch_outer's envelope: m in 4 .. 13, t in 1 .. 16, parity < n <= 2^m - 1."""

    def __init__(self, m, t, n=None):
        if not all(_is_int(x) for x in (m, t) + (() if n is None else (n,))):
            raise ValueError(f"BchCode takes integers, got m={m!r}, t={t!r}, n={n!r}")
        self.m, self.t = int(m), int(t)
        if not 4 <= self.m <= 13 or not 1 <= self.t <= 16:
            raise ValueError(f"BchCode: m in 4 .. 13 and t in 1 .. 16, got m={m}, t={t}")
        q = (1 << self.m) - 1
        seen = set()
        for j in range(1, 2 * self.t + 1):
            x = j % q
            while x not in seen:
                seen.add(x)
                x = 2 * x % q
        self.parity = len(seen)
        self.n = q if n is None else int(n)
        if not self.parity < self.n <= q:
            raise ValueError(f"BchCode({m}, {t}): {self.parity} parity bits need {self.parity} < n <= {q}, got n={self.n}")
        self.k = self.n - self.parity
        self.rate = self.k / self.n


def resolve_outer(outer, code=None):
    """ldpc_decode's outer= dict(code, payload=None, spread=True, codewords=None) with its defaults filled in; code: the LdpcCode in front, whose
    (nb - mb) Z is the default payload.  ValueError for an unknown key, a missing code or one that is no BchCode, a payload outside 1 .. n."""
    if not isinstance(outer, dict) or set(outer) - set(OUTER_KEYS) or not isinstance(outer.get("code"), BchCode):
        raise ValueError(f"outer takes a dict of {', '.join(OUTER_KEYS)} with a BchCode under code; got {sorted(outer) if isinstance(outer, dict) else outer!r}")
    payload = outer.get("payload")
    if payload is None and code is not None:
        payload = (code.nb - code.mb) * code.Z
    n = None if code is None else code.nb * code.Z             # (a column block of an ScLdpcCode is the codeword of the outer decoder's map)
    if payload is not None:
        payload = _payload(payload, n, f"outer['payload'] = {payload}: the first 1 .. n bits of a codeword")
    return dict(code=outer["code"], payload=payload, spread=bool(outer.get("spread", True)),
                codewords=outer.get("codewords"))


def bch_outer(post, bits, code, n, t0=0, depth=None, payload=None, spread=True, codewords=None, want_loc=False):
    """The hard-decision outer decoder behind ldpc_decode (vaeq_bch_outer): bounded-distance decoding of the BchCode `code` over the payload
    bits of post[R, C, n] (float32 or int16: ldpc_decode's post; a negative value is bit 1) against the TX bits `bits` ([R,2,2b,N] or [R,w,N],
    as for ldpc_decode, with its t0 and depth).  No encoder: the figures depend on the error pattern alone.  payload: the first K bits of every
    LDPC codeword are payload (default n: all of them; ldpc_decode's outer= defaults to (nb - mb) Z); the run's stream of C K bits holds
    `codewords` outer codewords (default C K // code.n; ValueError if none fits), bit-interleaved over the run if spread (position p of outer
    codeword a is stream bit p C_o + a) and back to back otherwise.
    -> dict(status, pre_err, bit_err, nflip [R,C_o] int64: status 0 = zero syndromes, 1 = corrected nflip <= t positions, 2 = detected and left
    alone; BER_outer[R], BER_in[R] f32 over the C_o n_o bits, FER_outer[R] the share of outer codewords with bit_err > 0; miscorrected[R]
    (status 1 with bit_err > 0) and undetected[R] (status 0 with pre_err > 0) int64; loc[R,C_o,t] int16, the flipped positions ascending and
    padded with -1, if want_loc)."""
    if not isinstance(code, BchCode):
        raise ValueError(f"bch_outer takes a BchCode, got {code!r}")
    if post.dim() != 3 or post.shape[2] != int(n) or post.dtype not in (torch.float32, torch.int16) or bits.dim() not in (3, 4) or bits.shape[0] != post.shape[0]:
        raise ValueError(f"expected post[R,C,{n}] float32 or int16 and bits[R,2,2b,N] or [R,w,N], got {tuple(post.shape)} {post.dtype}, {tuple(bits.shape)}")
    dev, R, C_, N = post.device, post.shape[0], post.shape[1], bits.shape[-1]
    post = post.contiguous()
    w = bits.shape[1] * (bits.shape[2] if bits.dim() == 4 else 1)
    bits = bits.reshape(R, w, N).contiguous()                  # (an empty batch leaves a -1 ambiguous)
    K = int(n) if payload is None else int(payload)
    _payload(K, int(n), f"payload = {K}: the first 1 .. {n} bits of a codeword")
    Co = C_ * K // code.n if codewords is None else int(codewords)
    if codewords is None and Co < 1:
        raise ValueError(f"no outer codeword of {code.n} bits fits into the {C_} x {K} payload bits of a run")
    out = torch.empty(R, max(Co, 0), 4, dtype=torch.int32, device=dev)
    loc = torch.empty(R, max(Co, 0), code.t, dtype=torch.int16, device=dev) if want_loc else None
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_bch_outer(R, C_, N, w, int(t0), 0 if depth is None else int(depth), int(n), K, code.m, code.t, code.n, Co,
                                           int(bool(spread)), nat.ptr(post, post.dtype), int(post.dtype == torch.int16), nat.ptr(bits, torch.int8),
                                           nat.ptr(out, torch.int32), nat.ptr(loc, torch.int16), nat.current_stream(dev)), "vaeq_bch_outer")
    o = out.long()
    ret = dict(_status_figures(o), BER_outer=_share(o[..., 2], Co * code.n), BER_in=_share(o[..., 1], Co * code.n),
               FER_outer=_share(o[..., 2] > 0, Co))
    if want_loc:
        ret["loc"] = loc
    return ret


class StaircaseCode:
    """A staircase code for staircase_decode: a chain of L blocks of s x s bits over the BchCode `component`, whose even length is 2 s.  Component
    j of pair i is the word [column j of block i - 1 | row j of block i]; block 0 is all zero and is not transmitted.  .component, .L, .s = n // 2,
    .n = L s^2 bits (n_chain), .rate = 1 - parity / s.  A rate of zero or below is allowed: that is a decoder test, not a code.  ValueError
    outside vaeq_staircase_decode's envelope: m in 4 .. 10, t in 1 .. 8, s in 2 .. 511, L in 1 .. 65535."""

    def __init__(self, component, L):
        if not isinstance(component, BchCode):
            raise ValueError(f"StaircaseCode takes a BchCode as its component, got {component!r}")
        if not _is_int(L) or not 1 <= int(L) <= 65535:
            raise ValueError(f"StaircaseCode: a chain of 1 .. 65535 blocks, got L={L!r}")
        if component.n % 2 or not 4 <= component.m <= 10 or not 1 <= component.t <= 8 or not 2 <= component.n // 2 <= 511:
            raise ValueError(f"StaircaseCode: a component with m in 4 .. 10, t in 1 .. 8 and an even n = 2 s, s in 2 .. 511; got m={component.m}, "
                             f"t={component.t}, n={component.n}")
        self.component, self.L, self.s = component, int(L), component.n // 2
        self.n = self.L * self.s * self.s
        self.rate = 1.0 - component.parity / self.s


def staircase_decode(llr, bits, code, window, t0=0, chains=None, iters=8, want_hard=False, want_profile=False):
    """Post-FEC figures of per-bit LLRs behind a hard-decision staircase code on the device (vaeq_staircase_decode): the hard decisions llr < 0
    against the TX bits give the error pattern of every chain of the StaircaseCode `code`; a window of `window` pairs of neighbouring blocks
    slides along the chain, and at each of the P = max(1, L - window + 1) positions the pairs inside are decoded component by component, at most
    `iters` times, until an iteration flips nothing.  llr, bits, t0 and the bit map as for ldpc_decode with n = code.n; chains: per run, default
    the most that fit behind t0.  No encoder: the figures depend on the error pattern alone.
    -> ldpc_sc_decode's dict, a chain where it has one (iters [R,C]: the sum over the positions; ok: at every position the last iteration found
    every component clean; bit_err, pre_err, erased, iters_max [R,C] int64; positions (P); BER_post[R], BER_pre[R], FER[R] f32), plus nflip and
    bad_flips [R,C] (all flips, and those of a bit that was right at that moment: what miscorrection costs).  want_hard: hard[R,C,n] int8, the
    final decisions.  want_profile: pos_err [R,C,L] (the errors of each block in its final state; the last block has one component per bit and
    keeps more than the steady state) and pos_iters [R,C,P]."""
    if not isinstance(code, StaircaseCode):
        raise ValueError(f"staircase_decode takes a StaircaseCode, got {code!r}")
    dev, R, N, w, llr, bits = _frame(llr, bits)
    n = code.n
    C_ = _count(chains, "chain", N, w, n, t0, None)
    P = max(1, code.L - int(window) + 1)
    Cn = max(C_, 0)
    out = torch.empty(R, Cn, 8, dtype=torch.int32, device=dev)
    hard = torch.empty(R, Cn, n, dtype=torch.int8, device=dev) if want_hard else None
    pos_err = torch.empty(R, Cn, code.L, dtype=torch.int32, device=dev) if want_profile else None
    pos_iters = torch.empty(R, Cn, P, dtype=torch.int32, device=dev) if want_profile else None
    bch = code.component
    with torch.cuda.device(dev):
        nat.check(nat.lib().vaeq_staircase_decode(R, C_, N, w, int(t0), bch.m, bch.t, code.s, code.L, nat.ptr(llr), nat.ptr(bits, torch.int8),
                                                  int(window), int(iters), nat.ptr(out, torch.int32), nat.ptr(hard, torch.int8),
                                                  nat.ptr(pos_err, torch.int32), nat.ptr(pos_iters, torch.int32), nat.current_stream(dev)),
                  "vaeq_staircase_decode")
    o, ret = _figures(out, C_, n, P)
    ret.update(nflip=o[..., 6], bad_flips=o[..., 7])
    if want_hard:
        ret["hard"] = hard
    if want_profile:
        ret["pos_err"], ret["pos_iters"] = pos_err.long(), pos_iters.long()
    return ret


class HammingCode:
    """A single-error-correcting code for chase_decode, given by the columns of its parity-check matrix: cols[n], column j an r-bit integer.
    .n, .r, .cols (int32), .rank (of the columns over GF(2)), .k = n - rank, .rate = k / n.  ValueError outside vaeq_chase_decode's envelope: n in
    3 .. 256, r in 2 .. 10, integer columns that are distinct, non-zero and below 2^r.  hamming_code builds the two textbook families; a standard's
    own matrix (the OIF 400ZR (128,119) word among them) is not in this package: a user who has its columns passes them here."""

    def __init__(self, cols, r):
        if not _is_int(r) or not 2 <= int(r) <= 10:
            raise ValueError(f"HammingCode: r in 2 .. 10, got {r!r}")
        c = np.asarray(cols)
        if c.ndim != 1 or not 3 <= c.size <= 256 or c.dtype == bool or not np.issubdtype(c.dtype, np.integer):
            raise ValueError(f"HammingCode: 3 .. 256 integer columns, got {c.dtype} of shape {c.shape}")
        if (c < 1).any() or (c >= 1 << int(r)).any() or np.unique(c).size != c.size:
            raise ValueError(f"HammingCode: the columns are distinct, non-zero and below 2^{int(r)}")
        self.cols, self.n, self.r = np.ascontiguousarray(c.astype(np.int32)), int(c.size), int(r)
        basis = {}                                             # leading bit -> a reduced column: Gaussian elimination over GF(2)
        for x in (int(v) for v in self.cols):
            while x and x.bit_length() in basis:
                x ^= basis[x.bit_length()]
            if x:
                basis[x.bit_length()] = x
        self.rank = len(basis)
        self.k = self.n - self.rank
        self.rate = self.k / self.n


def hamming_code(m, extended=True, n=None):
    """The HammingCode of the textbook column rules, shortened to its first n columns: extended (d = 4): r = m + 1, cols[j] = (j << 1) | 1,
    n <= 2^m (the default); plain (d = 3): r = m, cols[j] = j + 1, n <= 2^m - 1 (the default).  hamming_code(7) is the extended (128, 120) code,
    hamming_code(3, extended=False) the perfect (7, 4) code.  .k = n - r wherever the kept columns have rank r.  This is NOT the (128, 119) matrix of
    the OIF 400ZR agreement, which this package does not hold: pass its columns to HammingCode."""
    if not _is_int(m) or (n is not None and not _is_int(n)):
        raise ValueError(f"hamming_code takes integers, got m={m!r}, n={n!r}")
    m, full = int(m), (1 << int(m)) - (0 if extended else 1) if 1 <= int(m) <= 10 else 0
    n = full if n is None else int(n)
    if not 1 <= n <= full:
        raise ValueError(f"hamming_code({m}, extended={bool(extended)}): n in 1 .. {full}, got {n}")
    j = np.arange(n, dtype=np.int64)
    return HammingCode((j << 1) | 1 if extended else j + 1, m + 1 if extended else m)


class EbchCode:
    """An (extended) double-error-correcting BCH code for chase_decode and ProductCode (vaeq_chase_bch_decode): vaeq_bch_outer's narrow-sense
    primitive binary BCH code over GF(2^m) with designed correction t = 2, shortened to n_i inner bits and, where `extended`, followed by one
    overall parity bit: n = n_i + extended (default the full length, 2^m - 1 + extended).  .m, .n, .n_i, .extended, .k = n_i - 2 m,
    .rate = k / n.  EbchCode(7) is the extended (128, 113) word, d = 6.  ValueError outside the envelope: m in 4 .. 8, 2 m < n_i <= 2^m - 1.
    t = 3 and beyond are out of scope."""

    def __init__(self, m, n=None, extended=True):
        if not _is_int(m) or (n is not None and not _is_int(n)):
            raise ValueError(f"EbchCode takes integers, got m={m!r}, n={n!r}")
        if not 4 <= int(m) <= 8:
            raise ValueError(f"EbchCode: m in 4 .. 8, got {m!r}")
        ext = int(bool(extended))
        m, n = int(m), (1 << int(m)) - 1 + ext if n is None else int(n)
        if not 2 * m < n - ext <= (1 << m) - 1:
            raise ValueError(f"EbchCode(m={m}, extended={bool(ext)}): n in {2 * m + 1 + ext} .. {(1 << m) - 1 + ext}, got {n}")
        self.m, self.n, self.n_i, self.extended = m, n, n - ext, bool(ext)
        self.k = self.n_i - 2 * m
        self.rate = self.k / self.n

    def __repr__(self):
        return f"EbchCode(m={self.m}, n={self.n}, extended={self.extended})"


def ebch_code(m, extended=True, n=None):
    """The EbchCode over GF(2^m), shortened to n bits in all (the parity bit included), in the style of hamming_code: ebch_code(5) is the extended
    (32, 21) word, ebch_code(4, extended=False) the (15, 7) code, ebch_code(8, n=201) the inner 200 bits of the (255, 239) code and a parity bit."""
    return EbchCode(m, n, extended)


def chase_decode(llr, bits, code, t0=0, codewords=None, depth=None, patterns=4, payload=None, spread=True, want_stream=False):
    """The soft-in / hard-out inner decoder in front of the hard-decision FEC (vaeq_chase_decode; vaeq_chase_bch_decode where `code` is an
    EbchCode, whose test patterns are completed by bounded-distance decoding of up to two errors and the parity bit): Chase decoding of `code` over
    per-bit LLRs against the TX bits (no encoder: the rule acts on the error pattern).  llr, bits, t0, depth and the bit map as for ldpc_decode with
    n = code.n; codewords: per run, default the most that fit behind t0.  patterns = p in 0 .. min(6, n): the 2^p test patterns over the p least
    reliable positions, each completed by syndrome decoding; the candidate with the smallest sum of |llr| over its flips wins.  p = 0 is plain
    syndrome decoding of the hard decisions.  payload: the first K bits of every codeword (default code.k).
    -> dict(status, pre_err, bit_err, nflip, erased, pay_err [R,C] int64: status 0 = zero syndrome, 1 = flipped nflip bits, 2 = no candidate,
    left alone; bit_err the errors after decoding over the n bits, pay_err those among the payload; BER_post[R], BER_pre[R] over the C n bits,
    BER_payload[R] over the C K payload bits, FER[R] the share of codewords with bit_err > 0, f32; miscorrected[R] (status 1 with bit_err > 0) and
    undetected[R] (status 0 with pre_err > 0) int64).  want_stream: stream = dict(llr[R,1,C K] f32, bits[R,1,C K] int8), the decided payload
    bits as +-1.0 and their TX bits, codeword after codeword or, with spread, bit-interleaved over the run (payload bit i of codeword c at
    i C + c): a valid input of every decoder here with t0 = 0, which is how staircase_decode runs behind this one."""
    if not isinstance(code, (HammingCode, EbchCode)):
        raise ValueError(f"chase_decode takes a HammingCode or an EbchCode, got {code!r}")
    dev, R, N, w, llr, bits = _frame(llr, bits)
    n = code.n
    C_ = _count(codewords, "codeword", N, w, n, t0, depth)
    K = code.k if payload is None else int(payload)
    _payload(K, n, f"payload = {K}: the first 1 .. {n} bits of a codeword")
    Cn = max(C_, 0)
    out = torch.empty(R, Cn, 6, dtype=torch.int32, device=dev)
    s_llr, s_bits = _stream(want_stream, R, Cn * K, dev)
    tail = (nat.ptr(llr), nat.ptr(bits, torch.int8), int(patterns), K, int(bool(spread)), nat.ptr(out, torch.int32), nat.ptr(s_llr),
            nat.ptr(s_bits, torch.int8), nat.current_stream(dev))
    with torch.cuda.device(dev):
        if isinstance(code, EbchCode):
            nat.check(nat.lib().vaeq_chase_bch_decode(R, C_, N, w, int(t0), 0 if depth is None else int(depth), code.m, n, int(code.extended), *tail),
                      "vaeq_chase_bch_decode")
        else:
            nat.check(nat.lib().vaeq_chase_decode(R, C_, N, w, int(t0), 0 if depth is None else int(depth), n, code.r,
                                                  code.cols.ctypes.data_as(C.c_void_p), *tail), "vaeq_chase_decode")
    o = out.long()
    ret = dict(_status_figures(o), erased=o[..., 4], pay_err=o[..., 5], BER_post=_share(o[..., 2], C_ * n), BER_pre=_share(o[..., 1], C_ * n),
               BER_payload=_share(o[..., 5], C_ * K), FER=_share(o[..., 2] > 0, C_))
    if want_stream:
        ret["stream"] = dict(llr=s_llr, bits=s_bits)
    return ret


class ProductCode:
    """A product code for tpc_decode: blocks of col.n x row.n bits whose columns are words of the HammingCode `col` and whose rows are words of
    the HammingCode `row`.  .col, .row, .n = col.n row.n, .k = col.k row.k, .rate = k / n.  ValueError for anything but two HammingCodes, or a
    block whose state passes the LDS bound of vaeq_tpc_decode (include/vaeq.h; the extended (128, 120)^2 block fits).  Or two EbchCodes, which
    may differ in m, n and extended (vaeq_tpc_bch_decode; the extended (128, 113)^2 block fits, the (256, 239)^2 block does not).  .bch says which.
    One code of each kind is a ValueError: a mixed product is out of scope."""

    def __init__(self, col, row):
        self.bch = isinstance(col, EbchCode) and isinstance(row, EbchCode)
        if not self.bch and (not isinstance(col, HammingCode) or not isinstance(row, HammingCode)):
            raise ValueError(f"ProductCode takes two HammingCodes or two EbchCodes, got {col!r} and {row!r}")
        self.col, self.row = col, row
        self.n, self.k = col.n * row.n, col.k * row.k
        self.rate = self.k / self.n
        fits = (nat.lib().vaeq_tpc_bch_lds_bytes(col.m, col.n, int(col.extended), row.m, row.n, int(row.extended)) if self.bch
                else nat.lib().vaeq_tpc_lds_bytes(col.n, col.r, row.n, row.r))
        if fits < 0:
            raise ValueError(f"ProductCode: the state of a block of {col.n} x {row.n} bits does not fit the LDS of a CU (vaeq_tpc_lds_bytes)")


TPC_ALPHA = (0.0, 0.2, 0.3, 0.5, 0.7, 0.9, 1.0, 1.0)          # Pyndiah's schedules per half-iteration, continued with 1
TPC_BETA = (0.2, 0.4, 0.6, 0.8, 1.0, 1.0)
TPC_CLIP = 2.0 ** 60


def _tpc_schedule(name, given, default, iters, hi):
    """-> float32[2 iters]: `given` (2 iters values) or the default continued with 1; ValueError outside vaeq_tpc_decode's bounds."""
    if given is None:
        v = np.array((list(default) + [1.0] * (2 * iters))[:2 * iters], np.float32)
    else:
        try:
            v = np.ascontiguousarray(np.asarray(given, dtype=np.float32).reshape(-1))
        except (TypeError, ValueError):
            raise ValueError(f"{name}: 2 iters = {2 * iters} numbers, got {given!r}") from None
    if v.shape != (2 * iters,) or not np.isfinite(v).all() or (v < 0).any() or (hi is not None and (v > hi).any()):
        raise ValueError(f"{name}: 2 iters = {2 * iters} finite values in [0, {'inf' if hi is None else hi}{')' if hi is None else ']'}, got {given!r}")
    return v


def resolve_tpc(code, iters=4, patterns=4, alpha=None, beta=None, clip=None, payload=None):
    """tpc_decode's host-side arguments with their defaults filled in -> dict(iters, patterns, alpha, beta (float32[2 iters]), clip, payload
    (K1, K2)).  ValueError outside vaeq_tpc_decode's bounds."""
    if not isinstance(code, ProductCode):
        raise ValueError(f"tpc_decode takes a ProductCode, got {code!r}")
    for name, v, lo, hi in (("iters", iters, 1, 16), ("patterns", patterns, 0, min(6, code.col.n, code.row.n))):
        if not _is_int(v) or not lo <= v <= hi:
            raise ValueError(f"{name} = {v!r}: an integer in {lo} .. {hi}")
    iters = int(iters)
    clip = TPC_CLIP if clip is None else clip
    if not isinstance(clip, numbers.Real) or isinstance(clip, bool) or not math.isfinite(clip) or not 0 < clip <= 2.0 ** 96:
        raise ValueError(f"clip = {clip!r}: finite, in (0, 2^96]")
    K = (code.col.k, code.row.k) if payload is None else payload
    if (not isinstance(K, (tuple, list)) or len(K) != 2 or not all(_is_int(v) for v in K)
            or not 1 <= K[0] <= code.col.n or not 1 <= K[1] <= code.row.n):
        raise ValueError(f"payload = {K!r}: (K1, K2), the first 1 .. {code.col.n} rows and 1 .. {code.row.n} columns of a block")
    return dict(iters=iters, patterns=int(patterns), alpha=_tpc_schedule("alpha", alpha, TPC_ALPHA, iters, 16.0),
                beta=_tpc_schedule("beta", beta, TPC_BETA, iters, None), clip=float(clip), payload=(int(K[0]), int(K[1])))


def tpc_decode(llr, bits, code, t0=0, blocks=None, iters=4, patterns=4, alpha=None, beta=None, scale=None, clip=None, payload=None,
               want_stream=False, want_ext=False, want_profile=False):
    """Post-FEC figures of per-bit LLRs behind a soft-decision turbo product code on the device (vaeq_tpc_decode): Chase-Pyndiah decoding of the
    ProductCode `code`, rows in the even half-iterations and columns in the odd ones, at most 2 iters of them, each word by a Chase decoder over
    2^patterns test patterns whose competing candidates give the extrinsic values (vaeq_tpc_bch_decode where the code holds two EbchCodes: the same
    rule over double-error-correcting words).  llr, bits, t0 and the bit map as for ldpc_decode with
    n = code.n; blocks: per run, default the most that fit behind t0.  No encoder: the rule is stated on the LLRs towards the TX bits.
    alpha, beta: 2 iters values per half-iteration, default Pyndiah's schedules (0, .2, .3, .5, .7, .9, 1, 1 and .2, .4, .6, .8, 1, 1, continued
    with 1).  scale: per run ([R] tensor or a number), the unit of beta; default the float32 mean of |llr| over the run's tensor, non-finite
    entries counted as 0, formed on the device without a host synchronisation.  Unlike min-sum LDPC decoding the result depends on the scale of
    the LLRs.  clip: the bound of |r| and |W|, default 2^60.  payload = (K1, K2): the first rows and columns of a block, default (col.k, row.k).
    -> staircase_decode's common keys (iters [R,C]: half-iterations executed; ok: stopped on a product codeword; bit_err, pre_err, erased [R,C]
    int64; BER_post[R], BER_pre[R], FER[R] f32) plus pay_err, nstat2 (words without a candidate), nbeta (positions without a competitor) [R,C],
    BER_payload[R] over the C K1 K2 payload bits, and the resolved alpha, beta (tuples of float), scale ([R] f32) and clip.  want_stream:
    stream = dict(llr[R,1,C n] f32, bits[R,1,C n] int8), the decided bits as +-1.0 and their TX bits, a valid input of every decoder here with
    t0 = 0.  want_ext: ext[R,C,n] f32, the extrinsic values after the last executed half-iteration.  want_profile: half_err[R,C,2 iters] int64,
    the errors after each executed half-iteration, -1 behind the stop."""
    prm = resolve_tpc(code, iters, patterns, alpha, beta, clip, payload)
    dev, R, N, w, llr, bits = _frame(llr, bits)
    n = code.n
    C_ = _count(blocks, "block", N, w, n, t0, None)
    if scale is None:
        scale = torch.where(torch.isfinite(llr), llr.abs(), torch.zeros((), dtype=llr.dtype, device=dev)).mean(dim=(1, 2), dtype=torch.float32)
    elif not torch.is_tensor(scale):
        scale = torch.full((R,), float(scale), dtype=torch.float32, device=dev)
    scale = scale.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    if scale.shape != (R,):
        raise ValueError(f"scale: one value per run, [{R}], got {tuple(scale.shape)}")
    Cn, H = max(C_, 0), 2 * prm["iters"]
    out = torch.empty(R, Cn, 8, dtype=torch.int32, device=dev)
    s_llr, s_bits = _stream(want_stream, R, Cn * n, dev)
    ext = torch.empty(R, Cn, n, dtype=torch.float32, device=dev) if want_ext else None
    half = torch.empty(R, Cn, H, dtype=torch.int32, device=dev) if want_profile else None
    K1, K2 = prm["payload"]
    tail = (nat.ptr(llr), nat.ptr(bits, torch.int8), prm["patterns"], prm["iters"], prm["alpha"].ctypes.data_as(C.c_void_p),
            prm["beta"].ctypes.data_as(C.c_void_p), nat.ptr(scale) if R else None, prm["clip"], K1, K2, nat.ptr(out, torch.int32), nat.ptr(s_llr),
            nat.ptr(s_bits, torch.int8), nat.ptr(ext), nat.ptr(half, torch.int32), nat.current_stream(dev))
    with torch.cuda.device(dev):
        if code.bch:
            nat.check(nat.lib().vaeq_tpc_bch_decode(R, C_, N, w, int(t0), code.col.m, code.col.n, int(code.col.extended), code.row.m, code.row.n,
                                                    int(code.row.extended), *tail), "vaeq_tpc_bch_decode")
        else:
            nat.check(nat.lib().vaeq_tpc_decode(R, C_, N, w, int(t0), code.col.n, code.col.r, code.col.cols.ctypes.data_as(C.c_void_p), code.row.n,
                                                code.row.r, code.row.cols.ctypes.data_as(C.c_void_p), *tail), "vaeq_tpc_decode")
    o, ret = _figures(out, C_, n)
    ret.update(pay_err=o[..., 5], nstat2=o[..., 6], nbeta=o[..., 7], BER_payload=_share(o[..., 5], C_ * K1 * K2),
               alpha=tuple(float(v) for v in prm["alpha"]), beta=tuple(float(v) for v in prm["beta"]), scale=scale, clip=prm["clip"])
    if want_stream:
        ret["stream"] = dict(llr=s_llr, bits=s_bits)
    if want_ext:
        ret["ext"] = ext
    if want_profile:
        ret["half_err"] = half.long()
    return ret


INNER_KEYS = ("code", "patterns", "depth", "payload", "spread")
FEC_KEYS = ("code", "t0", "max_iter", "alpha", "depth", "quant", "window", "iters", "test", "fixed", "outer")
FEC_BLOCK_ONLY, FEC_SC_ONLY = ("max_iter", "depth", "quant"), ("window", "iters", "test", "fixed")
FEC_STAIRCASE_KEYS = ("code", "window", "t0", "iters")
FEC_TPC_KEYS = ("code", "t0", "iters", "patterns", "alpha", "beta", "scale", "clip")


def resolve_inner(inner):
    """The inner= dict(code=HammingCode or EbchCode, patterns=4, depth=None, payload=None, spread=True) of a fec= with a StaircaseCode, its defaults
    filled in.  ValueError for an unknown key, a missing code or one of another kind, patterns outside 0 .. min(6, n), a payload outside 1 .. n (or a
    code without a payload bit where none is given), a depth below 1."""
    if not isinstance(inner, dict) or set(inner) - set(INNER_KEYS) or not isinstance(inner.get("code"), (HammingCode, EbchCode)):
        raise ValueError(f"inner takes a dict of {', '.join(INNER_KEYS)} with a HammingCode or an EbchCode under code; got {sorted(inner) if isinstance(inner, dict) else inner!r}")
    code = inner["code"]
    patterns, payload, depth = inner.get("patterns", 4), inner.get("payload"), inner.get("depth")
    payload = code.k if payload is None else payload
    refusal = lambda name, v, lo, hi: f"inner[{name!r}] = {v!r}: an integer in {lo} .. {hi}"
    if not _is_int(patterns) or not 0 <= patterns <= min(6, code.n):
        raise ValueError(refusal("patterns", patterns, 0, min(6, code.n)))
    payload = _payload(payload, code.n, refusal("payload", payload, 1, code.n), whole=True)
    if depth is not None and (not _is_int(depth) or depth < 1):
        raise ValueError(refusal("depth", depth, 1, ""))
    return dict(code=code, patterns=int(patterns), depth=None if depth is None else int(depth), payload=payload, spread=bool(inner.get("spread", True)))


def _check_ldpc(fec):
    for key in ("quant", "fixed"):                              # the fixed-point rule: quant with an LdpcCode, fixed with an ScLdpcCode
        if fec.get(key) is not None:
            resolve_quant(fec[key])
            if fec.get("alpha") is not None:
                raise ValueError(f"fec takes alpha for the float decoder or {key} for the fixed-point one, not both")
    if fec.get("outer") is not None:
        resolve_outer(fec["outer"], fec["code"])


# The fec= dict by the class of its code: (the keys it takes, those it needs besides code, the check of their values, the decoder's name in
# this module: fec_figures looks it up when it runs).
_FEC_TABLE = {
    LdpcCode: (tuple(k for k in FEC_KEYS if k not in FEC_SC_ONLY), (), _check_ldpc, "ldpc_decode"),
    ScLdpcCode: (tuple(k for k in FEC_KEYS if k not in FEC_BLOCK_ONLY), ("window",), _check_ldpc, "ldpc_sc_decode"),
    StaircaseCode: (FEC_STAIRCASE_KEYS + ("inner",), ("window",), lambda fec: fec.get("inner") is None or resolve_inner(fec["inner"]),
                    "staircase_decode"),
    ProductCode: (FEC_TPC_KEYS, (), lambda fec: resolve_tpc(**{k: fec[k] for k in FEC_TPC_KEYS if k not in ("t0", "scale") and fec.get(k) is not None}),
                  "tpc_decode")}


def _fec_checked(fec):
    """check_fec of a fec= that is not None -> (the class of its code in _FEC_TABLE, the name of its decoder)."""
    code = fec.get("code") if isinstance(fec, dict) else None
    cls = next((c for c in _FEC_TABLE if isinstance(code, c)), LdpcCode)       # a code of no class here goes the LdpcCode's way
    keys, required, check, decoder = _FEC_TABLE[cls]
    unknown, missing = set(fec) - set(keys), [k for k in required if fec.get(k) is None]
    if cls is ProductCode and unknown:
        raise ValueError(f"fec with a ProductCode takes {', '.join(FEC_TPC_KEYS)}; got {sorted(fec)}")
    if cls is StaircaseCode and (unknown or missing):
        raise ValueError(f"fec with a StaircaseCode takes {', '.join(FEC_STAIRCASE_KEYS)}, inner, window required; got {sorted(fec)}")
    if unknown - set(FEC_KEYS) or "code" not in fec:            # the two LDPC classes share FEC_KEYS and name a key of the other class apart
        raise ValueError(f"fec takes {', '.join(FEC_KEYS)}; got {sorted(fec)}")
    if unknown:
        raise ValueError(f"fec with an {cls.__name__} does not take {', '.join(k for k in FEC_KEYS if k in unknown)}")
    if missing:
        raise ValueError("fec with an ScLdpcCode needs window, the row-block positions inside the decoding window")
    check(fec)
    return cls, decoder


def check_fec(fec):
    """ValueError for a fec= dict that fec_figures would refuse (None passes): for a runner to call before it allocates or launches anything."""
    if fec is not None:
        _fec_checked(fec)


def _cat_figures(parts):
    """The dicts of the chunks of a batch as one: tensors joined along the runs, nested dicts likewise, anything else (the resolved quant) once."""
    first = parts[0]
    return {k: torch.cat([p[k] for p in parts]) if torch.is_tensor(v) else _cat_figures([p[k] for p in parts]) if k == "outer" else v
            for k, v in first.items()}


def fec_figures(llr, fec):
    """The batch runners' fec= : ldpc_decode of an "llr" dict (llr, bits) under fec = dict(code, t0, max_iter, alpha, depth, quant, outer; all but
    code optional; quant = dict(bits, ...) decodes in fixed point, vaeq_ldpc_decode_q; outer = dict(code=BchCode, ...) adds bch_outer's figures
    under "outer").  With an outer code the runs are walked in chunks whose `post` stays within OUTER_POST_BYTES; codewords are independent, so
    the figures are those of one call.  With an ScLdpcCode under code it is ldpc_sc_decode under fec = dict(code, window, t0, iters, alpha, test,
    fixed, outer; code and window required): max_iter, depth and quant are a ValueError there, as window, iters, test and fixed are with an
    LdpcCode.  fixed = dict(bits, ...), quant's format, is the window decoder's quant=: fixed point, vaeq_ldpc_sc_decode_q.  With a StaircaseCode
    under code it is staircase_decode, hard-decision FEC, under fec = dict(code, window, t0, iters; code and window required); every other key
    is a ValueError there, but for inner = dict(code=HammingCode or EbchCode, patterns=4, depth=None, payload=None, spread=True): the concatenated scheme,
    chase_decode on the LLRs behind t0 and the staircase code on its payload stream from 0 (as many chains as fit the C K stream bits).  The
    staircase's dict comes back with BER_pre the inner decoder's -- the channel's, what a sweep's BER_pre_fec column means -- and the inner
    decoder's dict under "inner".  With a ProductCode (of two HammingCodes or of two EbchCodes) under code it is tpc_decode, the soft-decision turbo
    product decoder, under fec = dict(code, t0, iters, patterns, alpha, beta, scale, clip; all but code optional); every other key is a
    ValueError there."""
    cls, decoder = _fec_checked(fec)
    decode, L, B = globals()[decoder], llr["llr"], llr["bits"]
    if cls is ProductCode:
        return decode(L, B, **{k: v for k, v in fec.items() if v is not None})
    if cls is StaircaseCode and fec.get("inner") is not None:
        inner = resolve_inner(fec["inner"])
        first = chase_decode(L, B, inner["code"], t0=fec.get("t0", 0), depth=inner["depth"], patterns=inner["patterns"],
                             payload=inner["payload"], spread=inner["spread"], want_stream=True)
        stream = first.pop("stream")
        ret = decode(stream["llr"], stream["bits"], **{k: v for k, v in fec.items() if k not in ("inner", "t0")})
        ret["BER_pre"], ret["inner"] = first["BER_pre"], first
        return ret
    if cls is StaircaseCode:
        return decode(L, B, **{k: v for k, v in fec.items() if k != "inner"})
    kw = {"quant" if k == "fixed" else k: v for k, v in fec.items() if k != "code"}
    if fec.get("outer") is None or L.shape[0] == 0:
        return decode(L, B, fec["code"], **kw)
    R, N, n = L.shape[0], L.shape[-1], fec["code"].n
    w = L.numel() // max(R * N, 1)
    C_ = int(kw["codewords"]) if kw.get("codewords") is not None else _fit(N, w, n, kw.get("t0", 0), kw.get("depth"))
    per_run = max(C_, 1) * n * (4 if kw.get("quant") is None else 2)
    step = max(1, int(OUTER_POST_BYTES) // per_run)
    return _cat_figures([decode(L[r:r + step], B[r:r + step], fec["code"], **kw) for r in range(0, R, step)])
