#!/usr/bin/env python3
"""Bank-conflict model of the AWGN wave kernel's two blocked tap-gradient phases (csrc/vaeq_awgn_wave.hip, P4a dL/dh and P5 dL/dw).

For a lane -> (group, part) mapping and a part stride it counts, per loop trip, the LDS passes of every 8-byte operand read: a read of
64 lanes is served as two half-waves of 32; within a half-wave the lanes that name the SAME dword are one access (broadcast), different
dwords on the same of the 64 banks serialise.  passes(read) = sum over the two half-waves of the maximum bank multiplicity.
Usage: python tools/lds_bank_model.py [B] [M]
       python tools/lds_bank_model.py dp_d3 | dp_tappair      (the DP wave kernel's D phase / tap-pair tap gradients at the baked B = 100)
       python tools/lds_bank_model.py dp_fir_carry | dp_du_carry | dp_d3_carry   (its FIR / dL/dU / D loops with the carried cells, against the plain loops)
"""
import sys
from collections import defaultdict


def wave_lph(n):
    lph = (n + 3) // 4 + 1
    while (lph & 31) not in (8, 24):
        lph += 1
    return lph


def passes(addrs):
    """addrs: list over the 64 lanes of a float2 index (None = idle lane: shadows a working lane of its half-wave)."""
    total = 0
    for h in range(2):
        banks = defaultdict(set)
        half = addrs[32 * h:32 * h + 32]
        base = next((a for a in half if a is not None), addrs[0])    # an idle lane shadows a working lane of its own half-wave
        for a in half:
            a = base if a is None else a
            for d in (2 * a, 2 * a + 1):
                banks[d % 64].add(d)
        total += max(len(s) for s in banks.values())
    return total


def model(B, M, lane_map_h, lane_map_w, nit_h=None, nit_w=None, gy_planar=False, verbose=True):
    mh = M // 2
    Mh = 2 * mh
    L = 2 * B
    nm = L - Mh
    Lph = wave_lph(2 * B + M - 1)
    Uph = B // 2 + 1
    NG0, NG1 = (mh + 1 + 3) // 4, (mh + 3) // 4
    NGH, NGW = NG0 + NG1, (M + 3) // 4
    # LDS float2 offsets of the arrays (bytes / 8), as awgn_wave_layout lays them out
    X = 0
    E = X + 4 * Lph
    U = E + 4 * Lph
    # ---- P4a
    T = nm >> 1
    Tm = (T + 1) >> 1
    PH = max(p for _, p in lane_map_h if p is not None) + 1
    nit = nit_h or (Tm + PH - 1) // PH
    assert nit * PH >= Tm, (nit, PH, Tm)
    reads_h = []
    for rd in range(7):
        addrs = []
        for g, p in lane_map_h:
            if g is None:
                addrs.append(None)
                continue
            par = 1 if g >= NG0 else 0
            a0 = 4 * (g - NG0 if par else g)
            m0 = p * nit
            ceA, ceB, n0 = par + Mh, par + Mh + 2, mh - a0 - 3
            d = n0 & 1
            eA = E + (ceA & 3) * Lph + (ceA >> 2) + m0
            eB = E + (ceB & 3) * Lph + (ceB >> 2) + m0
            uE = U + d * Uph + (n0 >> 1) + m0
            uO = U + (d ^ 1) * Uph + (n0 >> 1) + d + m0
            addrs.append([eA, eB, uE, uO, uE + 1, uO + 1, uE + 2][rd])
        reads_h.append(passes(addrs))
    # ---- P5
    Bp = B >> 1
    PW = max(p for _, p in lane_map_w if p is not None) + 1
    nitw = nit_w or (Bp + PW - 1) // PW
    assert nitw * PW >= Bp
    reads_w = []
    for rd in range(8):
        addrs = []
        for g, p in lane_map_w:
            if g is None:
                addrs.append(None)
                continue
            m0 = p * nitw
            xw = X + g + m0
            if gy_planar:
                gy = [U + m0, U + Bp + 8 + m0]      # two planar arrays (even / odd symbols)
            else:
                gy = [U + 2 * m0, U + 2 * m0 + 1]
            addrs.append([gy[0], gy[1], xw, xw + Lph, xw + 2 * Lph, xw + 3 * Lph, xw + 1, xw + Lph + 1][rd])
        reads_w.append(passes(addrs))
    if verbose:
        print(f"  dL/dh: {PH} parts x {nit} trips, passes per read {reads_h} -> {sum(reads_h)} per trip, {sum(reads_h) * nit} per step (ideal {14 * nit})")
        print(f"  dL/dw: {PW} parts x {nitw} trips, passes per read {reads_w} -> {sum(reads_w)} per trip, {sum(reads_w) * nitw} per step (ideal {16 * nitw})")
    return sum(reads_h) * nit, sum(reads_w) * nitw


def group_major(NG, P):
    out = []
    for gl in range(64):
        g, p = gl // P, gl % P
        out.append((g, p) if g < NG else (None, None))
    return out


def half_split(NG, P):
    """parts 0..P/2-1 in the first half-wave, the rest in the second; group-minor inside a part"""
    out = [(None, None)] * 64
    hp = P // 2
    for p in range(P):
        h, pp = divmod(p, hp)
        for g in range(NG):
            out[32 * h + pp * NG + g] = (g, p)
    return out


def half_passes(addrs):
    """addrs: a float2 index for each of the 64 lanes (shadow lanes carry the address they really read) -> LDS passes of either half-wave"""
    out = []
    for h in range(2):
        banks = defaultdict(set)
        for a in addrs[32 * h:32 * h + 32]:
            for d in (2 * a, 2 * a + 1):
                banks[d % 64].add(d)
        out.append(max(len(s) for s in banks.values()))
    return out


def dp_d3_model(B=100, M=25):
    """D phase (P3) of the DP wave kernel at the baked B = 100 (csrc/vaeq_dp_wave_kernel.h): passes per half-wave of the mu reads of a tap stage and
    of the six x / e cells, for the three-tau-per-lane mapping (D3Map) and for the plain one (lane l' < nq owns tau = 2l', 2l'+1 of both chi; the
    lanes beyond shadow lane 0).  Tap reads are one word per half-wave (chi = lane >> 5) resp. per wave: one pass.    python tools/lds_bank_model.py dp_d3"""
    mh = M // 2
    Mh = 2 * mh
    nm = 2 * B - Mh
    T = nm // 2
    Lph, Uph = wave_lph(2 * B + M - 1), B // 2 + 1
    X, E = 0, 2 * 4 * wave_lph(2 * B + M - 1)
    U = 2 * E
    worst = {}
    # three tau per lane: m = lane & 31 (m >= 30 shadows m = 0), chi = lane >> 5
    m3 = [(l & 31) if (l & 31) < (T + 2) // 3 else 0 for l in range(64)]
    chi = [l >> 5 for l in range(64)]
    uE = [U + (m & 1) * Uph + ((3 * m) >> 1) for m in m3]
    uO = [U + ((m & 1) ^ 1) * Uph + ((3 * m) >> 1) + (m & 1) for m in m3]
    mu = []
    for nu in range(2):
        for b in range((mh + 1) // 2):
            sl = (mh >> 1) - b
            for base, o in ((uO, sl - 1), (uE, sl), (uO, sl), (uE, sl + 1)):
                mu.append(max(half_passes([a + nu * 2 * Uph + o for a in base])))
    worst["new mu"] = max(mu)
    cells = []
    for k in range(6):
        off = []
        for l in range(64):
            m, q = m3[l], 2 * (m3[l] & 1)
            off.append(chi[l] * 4 * Lph + (Mh >> 2) + ((3 * m) >> 1) + ((q + k) & 3) * Lph + ((q + k) >> 2))
        cells.append(max(max(half_passes([X + o for o in off])), max(half_passes([E + o for o in off]))))
    worst["new x / e cells"] = max(cells)
    # plain mapping: lane l' < nq, the rest shadow lane 0
    nq = (nm + 3) // 4
    lq = [l if l < nq else 0 for l in range(64)]
    mu = []
    ph = mh & 1
    for nu in range(2):
        for b in range((mh + 1) // 2):
            sl = (mh >> 1) - b
            for o in (ph * Uph + sl, (ph ^ 1) * Uph + sl + ph, (ph ^ 1) * Uph + sl + ph - 1):
                mu.append(max(half_passes([U + nu * 2 * Uph + l + o for l in lq])))
    worst["plain mu"] = max(mu)
    cells = []
    for c in range(2):
        for i in range(4):
            ce = Mh + i
            cells.append(max(half_passes([X + (c * 4 + (ce & 3)) * Lph + l + (ce >> 2) for l in lq])))
    worst["plain x / e cells"] = max(cells)
    print(f"DP wave kernel, D phase, B = {B}, M = {M}: Lph = {Lph}, Uph = {Uph}; worst LDS passes per half-wave and read:")
    for k, v in worst.items():
        print(f"  {k:18s} {v}")
    return worst


def dp_tappair_model(B=100, M=25):
    """Tap-gradient phases (P4a dL/dh, P5 dL/dw) of the DP wave kernel at the baked B = 100 (csrc/vaeq_dp_wave_kernel.h): passes per half-wave of every
    per-lane read of a pair of terms, for the tap-pair mapping (TapPairMap: lane = (c, half, par, slot), read tap + carried tap) and for the plain one
    (lane = (tap, half), every operand read).  The trip index adds the same offset to every lane: one trip is the pattern of all.
    Exit status 1 if a read of the tap-pair mapping needs more passes than the worst read of the plain mapping.    python tools/lds_bank_model.py dp_tappair"""
    mh = M // 2
    Mh = 2 * mh
    Lph, Uph = wave_lph(2 * B + M - 1), B // 2 + 1
    X, E = 0, 2 * 4 * Lph
    U = 2 * E                                                  # gy aliases U: [o][B]
    nh, nw = (B - mh) // 4, B // 4                             # pairs per half
    se = ((M + 1) // 2 + 1) // 2
    ns = se + (M // 2 + 1) // 2
    ph = lambda c: (c & 3) * Lph + (c >> 2)
    worst = {}
    # tap pairs
    dh, dw = [[] for _ in range(6)], [[] for _ in range(6)]
    for lane in range(64):
        ix = (lane & 31) if (lane & 31) < 2 * ns else 0
        c, hf = int(ix >= ns), lane >> 5
        s = ix - c * ns
        par = int(s >= se)
        sl = s - par * se
        pt = hf ^ c                                            # dL/dh: chi = 1 takes the halves of the tau range the other way round (TapPairMap::part_h): with pt = hf the two chi of a half-wave collide on every e read (2 passes)
        e = E + c * 4 * Lph + pt * nh
        uA = U + (mh >> 1) - sl + pt * nh
        for k, a in enumerate((e + ph(par + Mh), e + ph(par + Mh + 2), uA, uA + 2 * Uph, uA + Uph, uA + 3 * Uph)):
            dh[k].append(a)
        kr = 2 * (2 * sl + 1) + par
        g = U + c * B + 2 * hf * nw
        x = X + hf * nw
        for k, a in enumerate((g, g + 1, x + ph(kr), x + 4 * Lph + ph(kr), x + ph(kr + 2), x + 4 * Lph + ph(kr + 2))):
            dw[k].append(a)
    worst["pairs dL/dh"] = [max(half_passes(a)) for a in dh]
    worst["pairs dL/dw"] = [max(half_passes(a)) for a in dw]
    # plain: lane = (tap tk = lane & 31 (tk >= M shadows tap 0), half)
    dh, dw = [[] for _ in range(8)], [[] for _ in range(8)]
    for lane in range(64):
        tk, hf = (lane & 31) if (lane & 31) < M else 0, lane >> 5
        par, aa = tk & 1, tk >> 1
        npA, npB = mh - aa, mh - aa + 1
        eA, eB = E + ph(par + Mh) + hf * nh, E + ph(par + Mh + 2) + hf * nh
        uA, uB = U + (npA & 1) * Uph + (npA >> 1) + hf * nh, U + (npB & 1) * Uph + (npB >> 1) + hf * nh
        for k, a in enumerate((eA, eA + 4 * Lph, uA, uA + 2 * Uph, eB, eB + 4 * Lph, uB, uB + 2 * Uph)):
            dh[k].append(a)
        g0 = U + 2 * hf * nw
        xA, xB = X + ph(tk) + hf * nw, X + ph(tk + 2) + hf * nw
        for k, a in enumerate((g0, g0 + 1, g0 + B, g0 + B + 1, xA, xA + 4 * Lph, xB, xB + 4 * Lph)):
            dw[k].append(a)
    worst["plain dL/dh"] = [max(half_passes(a)) for a in dh]
    worst["plain dL/dw"] = [max(half_passes(a)) for a in dw]
    print(f"DP wave kernel, tap gradients, B = {B}, M = {M}: Lph = {Lph}, Uph = {Uph}; LDS passes per half-wave of each per-lane read of one pair of terms:")
    for k, v in worst.items():
        print(f"  {k:12s} {v}   reads {len(v)}, passes {sum(v)}")
    ok = all(max(worst["pairs " + g]) <= max(worst["plain " + g]) for g in ("dL/dh", "dL/dw"))
    print("  the tap pairs need", "no more" if ok else "MORE", "passes per read than the plain mapping's worst read")
    return ok


def _carry_report(title, plain, carry):
    """plain / carry: {stage: [worst passes per half-wave of each per-lane read of that stage]} -> (plain, carry) totals per step; prints both."""
    tp, tc = sum(sum(v) for v in plain.values()), sum(sum(v) for v in carry.values())
    np_, nc = sum(len(v) for v in plain.values()), sum(len(v) for v in carry.values())
    wp, wc = max(max(v) for v in plain.values()), max(max(v) for v in carry.values())
    print(f"DP wave kernel, {title}: per-lane reads per step {np_} -> {nc}, passes per half-wave {tp} -> {tc}, worst read {wp} -> {wc}")
    return dict(plain_reads=np_, carry_reads=nc, plain_passes=tp, carry_passes=tc, plain_worst=wp, carry_worst=wc)


def _pair_cells(bases, B, M, Lph, first):
    """Per-lane sample reads of the symbol-pair loops (pair_fir, pair_du): lane l < B / 2 reads cells 4 l + 4 g + j, the lanes beyond shadow lane 0.
    first(g): the j a stage still reads.  -> {(array, stage): [passes]}; the left-over tap's cells are stage G."""
    G = M // 4
    lanes = [l if l < B // 2 else 0 for l in range(64)]
    ph = lambda c: (c & 3) * Lph + (c >> 2)
    out = {}
    for ai, base in enumerate(bases):
        for g in range(G):
            out[(ai, g)] = [max(half_passes([base + l + ph(4 * g + j) for l in lanes])) for j in first(g)]
        out[(ai, G)] = [max(half_passes([base + l + ph(c) for l in lanes])) for c in ([4 * G + 2] if first(G) == "carry" else [4 * G, 4 * G + 2])]
    return out


def dp_fir_carry_model(B=100, M=25):
    """FIR (P1) at the baked B = 100: the sample reads of pair_fir (six per stage and p) against pair_fir_carry's (stage g >= 1 and the left-over tap
    take cells j = 0, 1 resp. 4G from registers).  Tap reads are one word per wave.    python tools/lds_bank_model.py dp_fir_carry"""
    Lph = wave_lph(2 * B + M - 1)
    bases = [p * 4 * Lph for p in range(2)]
    plain = _pair_cells(bases, B, M, Lph, lambda g: range(6) if g < M // 4 else "plain")
    carry = _pair_cells(bases, B, M, Lph, lambda g: (range(6) if g == 0 else range(2, 6)) if g < M // 4 else "carry")
    return _carry_report(f"FIR, B = {B}, M = {M}, Lph = {Lph}", plain, carry)


def dp_du_carry_model(B=100, M=25):
    """dL/dU (P4b) at the baked B = 100: the same on the residual e, both chi.    python tools/lds_bank_model.py dp_du_carry"""
    Lph = wave_lph(2 * B + M - 1)
    E = 2 * 4 * Lph
    bases = [E + c * 4 * Lph for c in range(2)]
    plain = _pair_cells(bases, B, M, Lph, lambda g: range(6) if g < M // 4 else "plain")
    carry = _pair_cells(bases, B, M, Lph, lambda g: (range(6) if g == 0 else range(2, 6)) if g < M // 4 else "carry")
    return _carry_report(f"dL/dU, B = {B}, M = {M}, Lph = {Lph}", plain, carry)


def dp_d3_carry_model(B=100, M=25):
    """D phase (P3) at the baked B = 100, three tau per lane (D3Map): the four mu reads of a tap stage against the carried form's (stage b >= 1 takes
    d = 1, 2 from registers).    python tools/lds_bank_model.py dp_d3_carry"""
    mh = M // 2
    T = B - mh
    Lph, Uph = wave_lph(2 * B + M - 1), B // 2 + 1
    U = 2 * 2 * 4 * Lph
    m3 = [(l & 31) if (l & 31) < (T + 2) // 3 else 0 for l in range(64)]
    uE = [U + (m & 1) * Uph + ((3 * m) >> 1) for m in m3]
    uO = [U + ((m & 1) ^ 1) * Uph + ((3 * m) >> 1) + (m & 1) for m in m3]
    plain, carry = {}, {}
    for nu in range(2):
        for b in range((mh + 1) // 2):
            sl = (mh >> 1) - b
            reads = [max(half_passes([a + nu * 2 * Uph + o for a in base])) for base, o in ((uO, sl - 1), (uE, sl), (uO, sl), (uE, sl + 1))]
            plain[(nu, b)] = reads
            carry[(nu, b)] = reads if b == 0 else reads[:2]
    return _carry_report(f"D, B = {B}, M = {M}, Uph = {Uph}", plain, carry)


DP_CARRY = {"dp_fir_carry": dp_fir_carry_model, "dp_du_carry": dp_du_carry_model, "dp_d3_carry": dp_d3_carry_model}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in DP_CARRY:
        r = DP_CARRY[sys.argv[1]]()
        sys.exit(0 if r["carry_worst"] <= r["plain_worst"] and r["carry_passes"] <= r["plain_passes"] else 1)
    if len(sys.argv) > 1 and sys.argv[1] == "dp_d3":
        dp_d3_model()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "dp_tappair":
        sys.exit(0 if dp_tappair_model() else 1)
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 350
    M = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    mh = M // 2
    NGH, NGW = (mh + 4) // 4 + (mh + 3) // 4, (M + 3) // 4
    print(f"B = {B}, M = {M}: Lph = {wave_lph(2 * B + M - 1)}, groups dL/dh {NGH}, dL/dw {NGW}")
    print("shipped mapping (lane = group * parts + part, parts = 64 / groups):")
    model(B, M, group_major(NGH, 64 // NGH), group_major(NGW, 64 // NGW))
    print("same, gy planar:")
    model(B, M, group_major(NGH, 64 // NGH), group_major(NGW, 64 // NGW), gy_planar=True)
    for nit_h, nit_w in ((None, None), (24, 24), (22, 24), (22, 22), (23, 24)):
        for planar in (False, True):
            print(f"8 parts, 4 per half-wave, trips {nit_h}/{nit_w}, gy planar {planar}:")
            try:
                model(B, M, half_split(NGH, 8), half_split(NGW, 8), nit_h, nit_w, planar)
            except AssertionError as e:
                print("  n/a", e)
