// vaeq_wave.h -- building blocks shared by the wave-per-run kernels (vaeq_dp_wave.hip, vaeq_awgn_wave.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace vaeq {

// One wave per workgroup: LDS instructions of a wave execute in issue order, so a later ds_read of any lane sees an earlier
// ds_write of any other lane without a hardware wait.  What is needed is only that the COMPILER keeps that order --
// __syncthreads() would also emit s_waitcnt vmcnt(0) and stall every phase on the step's in-flight q/y stores.
__device__ __forceinline__ void wave_lds_sync() { asm volatile("" ::: "memory"); }

// NW wavefronts per run: phases are separated by s_barrier after an LDS-only wait -- the in-flight global stores of a step still
// never stall a phase (gfx950 backs off barriers; the compiler adds no vmcnt(0) in front of this one).
template <int NW>
__device__ __forceinline__ void sync_lds()
{
    if constexpr (NW == 1) wave_lds_sync();
    else asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Sum K per-wave values (already reduced over the wave's lanes) over the NW waves of a run, same order in every wave; red: K NW floats.
template <int NW, int K>
__device__ __forceinline__ void waves_sum(float (&v)[K], float *red, int lane, int wv)
{
    if constexpr (NW > 1) {
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < K; k++) red[k * NW + wv] = v[k];
        }
        sync_lds<NW>();
#pragma unroll
        for (int k = 0; k < K; k++) {
            float t = red[k * NW];
#pragma unroll
            for (int w = 1; w < NW; w++) t += red[k * NW + w];
            v[k] = t;
        }
    }
}

typedef float v2f __attribute__((ext_vector_type(2)));   // element-wise ops compile to v_pk_{add,mul,fma}_f32

// Complex MACs.  A complex accumulator is kept as TWO packed partial sums,  a = sum re(t) * v  and  b = sum im(t) * v  (t = tap,
// v = sample), so that every MAC is exactly two v_pk_fma_f32 whose scalar factor rides on op_sel: no swap, no negation, no
// v_mov in the inner loops.  The two are combined once at the end:  t * v = (a.x - b.y, a.y + b.x),  v * conj(t) = (a.x + b.y, a.y - b.x).
struct cacc { v2f a, b; };
__device__ __forceinline__ cacc cacc0() { return cacc{v2f{0.f, 0.f}, v2f{0.f, 0.f}}; }
__device__ __forceinline__ void cmac(cacc &c, float tr, float ti, float2 v)           // c += (tr, ti) (x) v
{
    const v2f vv = {v.x, v.y};
    c.a += tr * vv;
    c.b += ti * vv;
}
// The same MAC with tap and sample as 8-byte register pairs straight from LDS (lds2): the tap's two halves ride on op_sel of the pair, so
// nothing is moved.  cmul starts an accumulator (first tap of a sum) instead of adding to a zeroed one: no v_mov 0 per accumulator.
__device__ __forceinline__ void cmac(cacc &c, v2f t, v2f v)
{
    c.a += t.x * v;
    c.b += t.y * v;
}
__device__ __forceinline__ void cmul(cacc &c, v2f t, v2f v)
{
    c.a = t.x * v;
    c.b = t.y * v;
}
template <bool FIRST>
__device__ __forceinline__ void cmacf(cacc &c, v2f t, v2f v)
{
    if constexpr (FIRST) cmul(c, t, v);
    else cmac(c, t, v);
}
// One 8-byte LDS read that stays one ds_read_b64 (volatile: never fused with a neighbour).  gfx950 serves ds_read_b64 at 256 B/clk but the
// fused ds_read2_b64 at 128 B/clk (8 instead of 2 x 2 LDS cycles per wave, MI355X_MICROARCH.md LDS table), its 8-bit offsets cost extra address
// adds, and the backend copies the 4th dword of a 16-byte result before it can broadcast it into a v_pk_fma_f32.
// (the cast names the LDS address space: address-space inference leaves volatile accesses alone, they would become flat loads)
typedef const volatile __attribute__((address_space(3))) v2f lds_cv2f;
__device__ __forceinline__ v2f lds2(const float2 *p) { return *(lds_cv2f *)p; }
__device__ __forceinline__ v2f lds2(const float *p) { return *(lds_cv2f *)p; }
// ... and the 4-byte form: wherever a read from a clamped (always valid) address feeds a select or a short-circuit test, which the backend would
// otherwise sink into a branch of its own behind its own s_waitcnt lgkmcnt(0)
typedef const volatile __attribute__((address_space(3))) float lds_cvf;
__device__ __forceinline__ float ldsv(const float *p) { return *(lds_cvf *)p; }
__device__ __forceinline__ float2 f2(v2f v) { return make_float2(v.x, v.y); }
// Two TAPS that are 16-byte aligned neighbours in LDS, read from a wave-uniform address as ONE ds_read_b128 (volatile: never split, never fused): the same
// four LDS cycles as the two ds_read_b64, half the instructions the wave issues and half the entries against the 4-bit lgkmcnt.  lo2 / hi2 are the two
// 8-byte halves of the result where the read put them (subregisters, no copy).  A packed FMA can broadcast either dword of either half (op_sel on the
// even-aligned pair), but the backend copies the 4th dword with a v_mov_b32 before it does: cmac16 / cmul16 / cmacf16 are cmac / cmul / cmacf with the
// two instructions the backend emits for them spelled out, operand for operand -- d = t.x v + d with op_sel_hi:[0,1,1], d = t.y v + d with
// op_sel:[1,0,0] -- so that a half of a 16-byte read feeds them in place.  The product that starts a chain is the matching v_pk_mul_f32.  Same operations
// in the same order as the C++ forms, hence the same bits.  Used by the baked B = 100, M = 25 DP kernel alone.
typedef float v4f __attribute__((ext_vector_type(4)));
typedef const volatile __attribute__((address_space(3))) v4f lds_cv4f;
__device__ __forceinline__ v4f lds4(const float4 *p) { return *(lds_cv4f *)p; }
__device__ __forceinline__ v4f lds4(const float2 *p) { return *(lds_cv4f *)p; }
__device__ __forceinline__ v2f lo2(v4f q) { return __builtin_shufflevector(q, q, 0, 1); }
__device__ __forceinline__ v2f hi2(v4f q) { return __builtin_shufflevector(q, q, 2, 3); }
__device__ __forceinline__ void cmac16(cacc &c, v2f t, v2f v)
{
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(c.a) : "v"(t), "v"(v));
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0]" : "+v"(c.b) : "v"(t), "v"(v));
}
__device__ __forceinline__ void cmul16(cacc &c, v2f t, v2f v)
{
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(c.a) : "v"(t), "v"(v));
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0]" : "=v"(c.b) : "v"(t), "v"(v));
}
template <bool FIRST>
__device__ __forceinline__ void cmacf16(cacc &c, v2f t, v2f v)
{
    if constexpr (FIRST) cmul16(c, t, v);
    else cmac16(c, t, v);
}
// lds2 where the kernel can afford it (V), an ordinary load (free to fuse / reorder: fewer live registers) where it is register-starved
template <bool V>
__device__ __forceinline__ v2f lds2_if(const float2 *p)
{
    if constexpr (V) return lds2(p);
    const float2 t = *p;
    return v2f{t.x, t.y};
}

// Buffer addressing for the streamed rows: address = base (4 SGPRs, one descriptor per array and frame) + a per-lane byte offset (VGPR) + a
// per-row byte offset (SGPR, folded into the instruction): NO vector ALU work per store / load, no 64-bit row pointers to keep (or spill) in
// scalar registers.  A lane that must not store / load passes OOB as its offset: the access is dropped by the range check (loads return 0).
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t OOB = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *p, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);   // raw buffer, gfx9 dword 3
}
// AUX = the store's cache policy bits (gfx950: 1 = sc0, 2 = nt, 16 = sc1; 0 = the default policy)
template <int AUX = 0>
__device__ __forceinline__ void bst64(v2f v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff)
{
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, (int)voff, (int)soff, AUX);
}
template <int AUX = 0>
__device__ __forceinline__ void bst32(float v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff)
{
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v), r, (int)voff, (int)soff, AUX);
}
__device__ __forceinline__ void bst16(unsigned short v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff)
{
    __builtin_amdgcn_raw_buffer_store_b16(v, r, (int)voff, (int)soff, 0);
}
__device__ __forceinline__ void bst8(unsigned char v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff)
{
    __builtin_amdgcn_raw_buffer_store_b8(v, r, (int)voff, (int)soff, 0);
}
__device__ __forceinline__ float4 bld128(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff)
{
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0);
    return __builtin_bit_cast(float4, v);
}

// Two-deep software pipeline over n >= 1 stages: load(i, r) issues stage i's NR independent 8-byte LDS reads, fma(i, r, first) consumes them.
// Stage i + 1 is in flight while stage i computes (register sets A / B alternate, no copies), so a wave hides its own LDS latency instead of
// relying on the one other wave of its SIMD to be in an FMA burst at that moment.  Loads run up to two stages past the end (never consumed):
// the caller's load(i) must stay inside the LDS allocation for i < n + 2 -- that keeps the loop body free of conditional loads.
// PIPE = false: plain loop (load, compute, load, compute ...) for phases that cannot spare the second register set.
template <int NR, bool INIT, bool PIPE = true, class L, class F>
__device__ __forceinline__ void pipe2(int n, L load, F fma)
{
    if (!INIT && n <= 0) return;                       // (INIT: the caller guarantees n >= 1, stage 0 starts the accumulators)
    if constexpr (!PIPE) {
        v2f A[NR];
        load(0, A);
        fma(0, A, std::integral_constant<bool, INIT>{});
#pragma unroll 1
        for (int i = 1; i < n; i++) {
            load(i, A);
            fma(i, A, std::false_type{});
        }
        return;
    }
    v2f A[NR], B[NR];
    load(0, A);
    load(1, B);
    fma(0, A, std::integral_constant<bool, INIT>{});
    int i = 1;
#pragma unroll 1
    for (; i + 1 < n; i += 2) {                        // B holds stage i
        load(i + 1, A);
        fma(i, B, std::false_type{});
        load(i + 2, B);
        fma(i + 1, A, std::false_type{});
    }
    if (i < n) fma(i, B, std::false_type{});
}

// pipe2 for loops whose stage i + 1 consumes operands that stage i already holds (the carried cells): those stay where stage i's loads put them, in
// the OTHER register set, and are read there.  n >= 2 stages, n even.  loadF(r): every operand of stage 0;  loadM(i, r): the operands of stage i that
// are neither carried in nor carried on;  loadL(i, r): the cells stage i carries on to stage i + 1 (they overwrite the ones stage i - 1 carried on, in
// the same set);  fma0(r): stage 0;  stage(r, p, mid): stage i >= 1 with its own operands in r and the carried ones in p -- it consumes everything it
// needs of p FIRST, then calls mid() (the loadL into p), then does the rest: no operand is copied on the back edge.  pre() runs ahead of the last
// stage's FMAs (reads of what follows the loop), and the last stage's set is handed to post(r).  No load runs past stage n - 1.
// PIPE = false: load, compute, load, compute ... as in pipe2 (one stage's operands live at a time, plus the carried cells); pre() runs behind the last stage.
template <int NR, bool PIPE = true, class LF, class LM, class LL, class F0, class S, class PRE, class POST>
__device__ __forceinline__ void pipe2_carry(int n, LF loadF, LM loadM, LL loadL, F0 fma0, S stage, PRE pre, POST post)
{
    v2f A[NR], B[NR];
    loadF(A);
    if constexpr (!PIPE) {
        fma0(A);
        int i = 1;
#pragma unroll 1
        for (; i + 1 < n; i += 2) {
            loadM(i, B);
            loadL(i, B);
            stage(B, A, []() {});
            loadM(i + 1, A);
            loadL(i + 1, A);
            stage(A, B, []() {});
        }
        loadM(i, B);
        loadL(i, B);
        stage(B, A, []() {});
        pre();
        post(B);
        return;
    }
    loadM(1, B);
    loadL(1, B);
    fma0(A);
    int i = 1;
#pragma unroll 1
    for (; i + 1 < n; i += 2) {                        // B holds stage i, A what stage i - 1 carried on
        loadM(i + 1, A);
        stage(B, A, [&]() { loadL(i + 1, A); });
        loadM(i + 2, B);
        stage(A, B, [&]() { loadL(i + 2, B); });
    }
    pre();
    stage(B, A, []() {});
    post(B);
}

// Final combine of the two packed partial sums, ONE v_pk_add_f32 each: the swap of b's halves and the sign ride on op_sel / neg (the backend
// does not find this form: it shuffles the halves with v_mov and adds them as scalars).
__device__ __forceinline__ v2f cfin2(const cacc &c)                                    // sum t * v = (a.x - b.y, a.y + b.x)
{
    v2f r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(c.a), "v"(c.b));
    return r;
}
__device__ __forceinline__ v2f cfinc2(const cacc &c)                                   // sum v * conj(t) = (a.x + b.y, a.y - b.x)
{
    v2f r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(c.a), "v"(c.b));
    return r;
}
__device__ __forceinline__ float2 cfin(const cacc &c) { const v2f r = cfin2(c); return make_float2(r.x, r.y); }
__device__ __forceinline__ float2 cfinc(const cacc &c) { const v2f r = cfinc2(c); return make_float2(r.x, r.y); }

// Cross-lane sums on the vector ALU (DPP), no LDS round trips: a ds_bpermute butterfly costs six dependent LDS latencies (~100 cycles each under
// load) during which the wave issues nothing; the DP kernel has five such sums and three scans per step.  Fixed order => bitwise reproducible.
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF>
__device__ __forceinline__ float dpp_f(float v)           // lanes the masks switch off (or whose source lies outside the row) contribute 0
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, BANK_MASK, true));
}
__device__ __forceinline__ float wave_sum_dpp(float v)    // sum over the 64 lanes, result in every lane (uniform)
{
    v += dpp_f<0xB1>(v);                                   // quad_perm:[1,0,3,2]
    v += dpp_f<0x4E>(v);                                   // quad_perm:[2,3,0,1]
    v += dpp_f<0x141>(v);                                  // row_half_mirror
    v += dpp_f<0x140>(v);                                  // row_mirror: every lane of a 16-lane row holds the row's sum
    // the four row sums r0..r3 meet in lane 63 as (r3 + r2) + (r1 + r0) -- the same additions as (r0 + r1) + (r2 + r3) from four v_readlane (IEEE
    // addition commutes: bitwise the same result) with two DPP broadcasts and ONE v_readlane instead of four v_readlane and three adds
    v += dpp_f<0x142, 0xA>(v);                             // row_bcast:15 into rows 1 and 3: r1 + r0, r3 + r2
    v += dpp_f<0x143, 0xC>(v);                             // row_bcast:31 into rows 2 and 3: lane 63 = (r3 + r2) + (r1 + r0)
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float row_incl_scan_dpp(float v)   // inclusive prefix sum inside each 16-lane row
{
    float s = v + dpp_f<0x111>(v);                         // row_shr:1
    s += dpp_f<0x112>(v);                                  // row_shr:2
    s += dpp_f<0x113>(v);                                  // row_shr:3   -> sums of (up to) 4
    s += dpp_f<0x114, 0xF, 0xE>(s);                        // row_shr:4 into banks 1..3
    s += dpp_f<0x118, 0xF, 0xC>(s);                        // row_shr:8 into banks 2, 3
    return s;
}
__device__ __forceinline__ float half_incl_scan_dpp(float v)  // inclusive prefix sum inside each 32-lane half
{
    float s = row_incl_scan_dpp(v);
    s += dpp_f<0x142, 0xA>(s);                             // row_bcast:15 into rows 1 and 3
    return s;
}
__device__ __forceinline__ float wave_incl_scan_dpp(float v)  // inclusive prefix sum over the 64 lanes
{
    float s = half_incl_scan_dpp(v);
    s += dpp_f<0x143, 0xC>(s);                             // row_bcast:31 into rows 2 and 3
    return s;
}

// The same sums and scans with every row- or bank-masked step as ONE instruction, v_add_f32_dpp v, v, v <ctrl> <masks> with the destination tied to the
// input: a lane the masks switch off keeps v where the forms above compute v + 0 -- from update_dpp(0, ...) the backend makes v_mov_b32 t, 0 +
// v_mov_b32_dpp t, v + v_add_f32 v, v, t, because it may not fold x + 0 into x (x = -0).  Several independent chains are interleaved in one asm
// statement: the hazard recognizer does not look inside one, so the two wait states a DPP read of a just-written VGPR needs are spelled out -- the leading
// s_nop 4 covers whatever wrote the inputs (or, as a VALU instruction, EXEC), and between two steps of a chain stand the other chains' steps (plus s_nop 0 where there is only one other).
// What FOLLOWS such a statement is the compiler's again: it sees the statement's outputs as written by it and places the wait state that the v_readlane of
// wave_sum5_dpp_keep needs behind a VALU write of its source (an s_nop 0 or an independent instruction behind the statement, as the listing shows).
// Used by the baked B = 100 DP kernel alone; every other kernel keeps the forms above.
#define VAEQ_DPPK(i, ctrl) "v_add_f32_dpp %" #i ", %" #i ", %" #i " " ctrl "\n\t"
#define VAEQ_DPPK2(ctrl) VAEQ_DPPK(0, ctrl) VAEQ_DPPK(1, ctrl)
#define VAEQ_DPPK5(ctrl) VAEQ_DPPK2(ctrl) VAEQ_DPPK(2, ctrl) VAEQ_DPPK(3, ctrl) VAEQ_DPPK(4, ctrl)
#define VAEQ_DPP_FULL " row_mask:0xf bank_mask:0xf"
// First step of wave_sum_dpp (quad_perm:[1,0,3,2]) on a value / on a product a b.  The caller of wave_sum5_dpp_keep does it: where a product feeds
// wave_sum_dpp the backend contracts its first addition, v + dpp(v) with v = a b, into fma(a, b, dpp(round(a b))) -- part of the pinned bits, spelled out here.
__device__ __forceinline__ float wave_sum_first(float v) { return v + dpp_f<0xB1>(v); }
__device__ __forceinline__ float wave_sum_first(float a, float b) { return __builtin_fmaf(a, b, dpp_f<0xB1>(a * b)); }
// Steps 2..6 of wave_sum_dpp on five chains at once (v[k]: after wave_sum_first), the sums in v[k] (uniform).  The same additions in the same order
// as wave_sum_dpp for EVERY input: a row that a masked step switches off is never read again on the way to lane 63 (rows 0 and 2 are read by
// row_bcast:15 before it, row 1 by row_bcast:31 after it added row 0 into it, and only row 3's last lane leaves).
__device__ __forceinline__ void wave_sum5_dpp_keep(float (&v)[5])
{
    asm("s_nop 4\n\t"
        VAEQ_DPPK5("quad_perm:[2,3,0,1]" VAEQ_DPP_FULL)
        VAEQ_DPPK5("row_half_mirror" VAEQ_DPP_FULL)
        VAEQ_DPPK5("row_mirror" VAEQ_DPP_FULL)
        VAEQ_DPPK5("row_bcast:15 row_mask:0xa bank_mask:0xf")
        VAEQ_DPPK5("row_bcast:31 row_mask:0xc bank_mask:0xf")
        : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]));
#pragma unroll
    for (int k = 0; k < 5; k++) v[k] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[k]), 63));
}
// wave_incl_scan_dpp of two values at once.  A switched-off lane keeps its partial sum s instead of s + 0: the same bits unless s is -0 (-0 + 0 = +0).
// For inputs that are never -0 (only -0 + -0 is -0) no partial sum is: the caller shows that of its inputs.
__device__ __forceinline__ void wave_incl_scan2_dpp_keep(float &a, float &b)
{
    float s0 = a + dpp_f<0x111>(a), s1 = b + dpp_f<0x111>(b);                  // row_shr:1 .. 3: full masks, as in row_incl_scan_dpp
    s0 += dpp_f<0x112>(a); s1 += dpp_f<0x112>(b);
    s0 += dpp_f<0x113>(a); s1 += dpp_f<0x113>(b);
    asm("s_nop 4\n\t"
        VAEQ_DPPK2("row_shr:4 row_mask:0xf bank_mask:0xe") "s_nop 0\n\t"
        VAEQ_DPPK2("row_shr:8 row_mask:0xf bank_mask:0xc") "s_nop 0\n\t"
        VAEQ_DPPK2("row_bcast:15 row_mask:0xa bank_mask:0xf") "s_nop 0\n\t"
        VAEQ_DPPK2("row_bcast:31 row_mask:0xc bank_mask:0xf")
        : "+v"(s0), "+v"(s1));
    a = s0;
    b = s1;
}
#undef VAEQ_DPPK
#undef VAEQ_DPPK2
#undef VAEQ_DPPK5
#undef VAEQ_DPP_FULL

__device__ __forceinline__ float wave_incl_scan(float v, int lane)                    // inclusive prefix sum over lanes
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// polyphase-4 row length (in float2) for a sample-rate array of `len` cells: phase arrays end up 16 (mod 64) dwords apart, so
// the stride-4 reads of consecutive lanes are bank-conflict free
__host__ __device__ constexpr inline int wave_lph(int len)
{
    int lph = (len + 3) / 4 + 1;
    while ((lph & 31) != 8 && (lph & 31) != 24) lph++;
    return lph;
}

}  // namespace vaeq
