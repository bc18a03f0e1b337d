// vaeq_awgn_dfe.hip -- the known-channel ("genie") baselines of AWGN_channel/DFE_MQAM_shaping.py at 1 sample per symbol.
//
//   compl_conv (:236-241): four real conv1d of the rails with the flipped taps, padding K / 2: out[i] = sum_t x[i + t - K/2] h[K-1-t],
//   re = (xr.hr) - (xi.hi), im = (xi.hr) + (xr.hi).  N + 1 outputs for the 20-tap LMMSE, N for the 11-tap feed-forward filter.
//   nearest_neighbor (:224-234): per-axis slicing against the levels (index iI * n + iQ); it differs from the reference's argmin over all n^2
//   complex distances only where two float32 distances round equal.
//   dfe (:200-222): the first K2 decisions are the LMMSE decisions; then I_p = ff[p] + sum_j fb[j] state[p-1-j], hard decision, p = K2 .. N-1.
//
// lmmse_eval_kernel: one 1024-thread workgroup per frame: the LMMSE output (track + decisions), find_shift_symb(., ., n_shift) and SER_func
// with the one-sample-longer output slice (:279-282), through vaeq_awgn_eval.h.
// The DFE runs as exact speculate-and-repair ("The DFE kernel"):
//   dfe_ff_kernel     the feed-forward FIR of every symbol, in parallel -> ff[R][N] (float2);
//   dfe_spec_kernel   one lane per (frame, chunk c): chunk c = [s_c, s_c + CH) with s_c = K2 + c CH; the lane starts W symbols early from the
//                     LMMSE decisions (chunk 0: exactly the reference's start), writes its chunk's decisions and keeps the K2 decisions its
//                     warm-up ended with (the speculative state at s_c);
//   dfe_repair_kernel one wave per frame: lane 0 walks the chunks; where the true state at s_c differs from the speculative one it re-runs the
//                     recursion until K2 consecutive new decisions equal the stored ones (from there both trajectories coincide);
//   dfe_eval_kernel   find_shift_symb(., ., n_shift) and SER_func on the hard-decision track (:290-293).
// Both recursions call dfe_step, so the result is bit-identical to the serial recursion (C = 1) for every C and W.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vaeq.h"
#include "vaeq_awgn_eval.h"
#include "vaeq_common.h"
#include "vaeq_launch.h"

namespace vaeq {

constexpr int LE_NT = 1024;                                    // threads of the LMMSE / DFE evaluation workgroups
constexpr int DFE_KMAX = 64;                                   // longest LMMSE / feed-forward filter
constexpr int DFE_SPEC_B = 16;                                 // bytes per stored speculative state (K2 <= 10)
constexpr int DFE_CMAX = 8192;                                 // most chunks per frame (one LDS byte each in the repair kernel)
constexpr int DFE_AHEAD = 8;                                   // feed-forward samples in flight ahead of the recursion

// compl_conv output i of one run: taps in LDS as the flipped taps hf[2][K] (re, im); zero padding outside [0, N).
__device__ __forceinline__ float2 compl_conv_at(const float *x0, const float *x1, int N, int K, const float (*hf)[DFE_KMAX], int i)
{
    float a = 0.f, b = 0.f, c = 0.f, d = 0.f;                  // xr.hr, xi.hi, xi.hr, xr.hi
    const int s0 = i - K / 2;
    for (int t = 0; t < K; t++) {
        const int s = s0 + t;
        if (s >= 0 && s < N) {
            const float vr = x0[s], vi = x1[s];
            a = fmaf(vr, hf[0][t], a);
            b = fmaf(vi, hf[1][t], b);
            c = fmaf(vi, hf[0][t], c);
            d = fmaf(vr, hf[1][t], d);
        }
    }
    return make_float2(__fsub_rn(a, b), __fadd_rn(c, d));
}

// Per-axis nearest level (first index on ties) of a value, levels in registers.
template <int NL>
__device__ __forceinline__ int slice_reg(float y, const float (&lev)[NL], float &val)
{
    int c = 0;
    float b = fabsf(__fsub_rn(y, lev[0]));
    val = lev[0];
#pragma unroll
    for (int l = 1; l < NL; l++) {
        const float d = fabsf(__fsub_rn(y, lev[l]));
        if (d < b) { b = d; c = l; val = lev[l]; }
    }
    return c;
}

// Per-axis nearest level with the levels in memory (the LMMSE decisions, off any dependency chain).
__device__ __forceinline__ int slice_mem(float y, const float *lev, int n)
{
    int c = 0;
    float b = fabsf(__fsub_rn(y, lev[0]));
    for (int l = 1; l < n; l++) {
        const float d = fabsf(__fsub_rn(y, lev[l]));
        if (d < b) { b = d; c = l; }
    }
    return c;
}

// The DFE state: the last K2M decisions as level values (sr, si) and indices (ix); slot j holds the decision at p - 1 - j.  Slots j >= K2
// carry zero taps and zero values.
template <int K2M>
struct DfeState {
    float sr[K2M], si[K2M];
    int ix[K2M];
};

// ONE step of the recursion (:212-219), used by the speculative and the repair pass alike.  The correction is summed from the oldest decision
// to the newest (the newest enters last: the rest of the sum does not wait for it), every operation rounded as written.
template <int NL, int K2M>
__device__ __forceinline__ int dfe_step(float2 v, const float (&fr)[K2M], const float (&fi)[K2M], const float (&nfi)[K2M],
                                        DfeState<K2M> &st, const float (&lev)[NL])
{
    float cr = 0.f, ci = 0.f;
#pragma unroll
    for (int j = K2M - 1; j >= 0; j--) {
        cr = fmaf(fr[j], st.sr[j], cr);
        cr = fmaf(nfi[j], st.si[j], cr);
        ci = fmaf(fr[j], st.si[j], ci);
        ci = fmaf(fi[j], st.sr[j], ci);
    }
    float vr, vi;
    const int cI = slice_reg<NL>(__fadd_rn(v.x, cr), lev, vr);
    const int cQ = slice_reg<NL>(__fadd_rn(v.y, ci), lev, vi);
#pragma unroll
    for (int j = K2M - 1; j > 0; j--) {
        st.sr[j] = st.sr[j - 1];
        st.si[j] = st.si[j - 1];
        st.ix[j] = st.ix[j - 1];
    }
    const int d = cI * NL + cQ;
    st.sr[0] = vr;
    st.si[0] = vi;
    st.ix[0] = d;
    return d;
}

// Taps and levels of a run into registers.
template <int NL, int K2M>
__device__ __forceinline__ void dfe_setup(const float *fb, const float *amp, int K2, float (&fr)[K2M], float (&fi)[K2M], float (&nfi)[K2M],
                                          float (&lev)[NL])
{
#pragma unroll
    for (int l = 0; l < NL; l++) lev[l] = amp[l];
#pragma unroll
    for (int j = 0; j < K2M; j++) {
        fr[j] = j < K2 ? fb[j] : 0.f;
        fi[j] = j < K2 ? fb[K2 + j] : 0.f;
        nfi[j] = -fi[j];
    }
}

// The state in front of position p0 from the decisions dec[p0 - 1 - j], j < K2.  The level values come from amp in memory: this is not on
// the step-to-step chain, and a dynamic index into the level registers would go through scratch.
template <int NL, int K2M>
__device__ __forceinline__ void dfe_load_state(DfeState<K2M> &st, const int8_t *dec, int p0, int K2, const float *amp)
{
#pragma unroll
    for (int j = 0; j < K2M; j++) {
        const int d = j < K2 ? (int)(uint8_t)dec[p0 - 1 - j] : 0;
        st.ix[j] = d;
        st.sr[j] = j < K2 ? amp[min(d / NL, NL - 1)] : 0.f;
        st.si[j] = j < K2 ? amp[d % NL] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- LMMSE evaluation
__global__ __launch_bounds__(LE_NT) void lmmse_eval_kernel(int N, int K, int n_lev, int n_shift, int n_cut, const float *__restrict__ rx,
                                                           const float *__restrict__ taps, const float *__restrict__ amp,
                                                           const __half *__restrict__ data, float2 *__restrict__ track,
                                                           int8_t *__restrict__ dec, float *__restrict__ ser, int32_t *__restrict__ shift_out)
{
    __shared__ float hf[2][DFE_KMAX];
    __shared__ float red[LE_NT / 64];
    __shared__ float corr[2][64];
    __shared__ float lev[8];
    __shared__ int sh_shift;
    const int run = blockIdx.x, tid = threadIdx.x;
    const int No = N + 2 * (K / 2) - K + 1;                    // conv1d output length
    const float *x0 = rx + (size_t)run * 2 * N, *x1 = x0 + N;
    float2 *tr = track + (size_t)run * No;
    if (tid < K) {
        hf[0][tid] = taps[(size_t)run * 2 * K + K - 1 - tid];
        hf[1][tid] = taps[(size_t)run * 2 * K + K + K - 1 - tid];
    }
    if (tid < n_lev) lev[tid] = amp[tid];
    __syncthreads();
    // compl_conv (:236-241) and nearest_neighbor(out[1::1]) (:275)
    int8_t *dr = dec ? dec + (size_t)run * N : nullptr;
    for (int i = tid; i < No; i += LE_NT) {
        const float2 y = compl_conv_at(x0, x1, N, K, hf, i);
        tr[i] = y;
        if (dr && i >= 1 && i - 1 < N) dr[i - 1] = (int8_t)(slice_mem(y.x, lev, n_lev) * n_lev + slice_mem(y.y, lev, n_lev));
    }
    __syncthreads();
    // find_shift_symb(out, data, n_shift) (:280), SER_func(out[:, n_cut+11+shift : -11-n_cut], data[:, n_cut+11 : -11-shift-n_cut]) (:281)
    const __half *tx0 = data + (size_t)run * 2 * N, *tx1 = tx0 + N;
    auto trk = [&](int m) { return tr[m]; };
    const int shift = eval_find_shift<LE_NT>(trk, tx0, tx1, n_shift, No, corr, &sh_shift, tid);
    const int L = N - 22 - 2 * n_cut - shift, Lr = No - 22 - 2 * n_cut - shift;
    const float s = eval_ser<LE_NT>(trk, n_cut + 11 + shift, Lr, tx0 + n_cut + 11, tx1 + n_cut + 11, L, lev, n_lev, red, tid);
    if (tid == 0) {
        ser[run] = s;
        if (shift_out) shift_out[run] = shift;
    }
}

// ---------------------------------------------------------------------------------------------------------------- DFE
// Feed-forward FIR (:285) of every symbol: grid (ceil(N / 256), R).
__global__ __launch_bounds__(256) void dfe_ff_kernel(int N, int K, const float *__restrict__ rx, const float *__restrict__ taps,
                                                     float2 *__restrict__ ff)
{
    __shared__ float hf[2][DFE_KMAX];
    const int run = blockIdx.y, tid = threadIdx.x;
    if (tid < K) {
        hf[0][tid] = taps[(size_t)run * 2 * K + K - 1 - tid];
        hf[1][tid] = taps[(size_t)run * 2 * K + K + K - 1 - tid];
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;
    const float *x0 = rx + (size_t)run * 2 * N;
    if (i < N) ff[(size_t)run * N + i] = compl_conv_at(x0, x0 + N, N, K, hf, i);
}

// Speculative pass: lane = run * C + c.  Writes dec[run][s_c .. e_c) (chunk 0 also the K2 LMMSE decisions in front) and the state the
// lane held at s_c into spec[run][c][0 .. K2) (position s_c - K2 + q).
template <int NL, int K2M>
__global__ __launch_bounds__(256) void dfe_spec_kernel(int R, int N, int K2, int C, int CH, int W, const float2 *__restrict__ ff,
                                                       const float *__restrict__ fb, const float *__restrict__ amp,
                                                       const int8_t *__restrict__ init, int8_t *__restrict__ dec, int8_t *__restrict__ spec)
{
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= R * C) return;
    const int run = gid / C, c = gid - run * C;
    const int s = K2 + c * CH, e = min(N, s + CH);
    const int w0 = c == 0 ? K2 : max(K2, s - W);
    float fr[K2M], fi[K2M], nfi[K2M], lev[NL];
    dfe_setup<NL, K2M>(fb + (size_t)run * 2 * K2, amp, K2, fr, fi, nfi, lev);
    const int8_t *in = init + (size_t)run * N;
    int8_t *dr = dec + (size_t)run * N;
    DfeState<K2M> st;
    dfe_load_state<NL, K2M>(st, in, w0, K2, amp);              // :208-209: the LMMSE decisions in front of the first step
    if (c == 0)
        for (int q = 0; q < K2; q++) dr[q] = in[q];
    int8_t *sp = spec + ((size_t)run * C + c) * DFE_SPEC_B;
    const float2 *f = ff + (size_t)run * N;
    float2 q[DFE_AHEAD];                                       // the next feed-forward samples, in flight ahead of the recursion
#pragma unroll
    for (int d = 0; d < DFE_AHEAD; d++) q[d] = f[min(w0 + d, e - 1)];
    for (int p0 = w0; p0 < e; p0 += DFE_AHEAD) {
#pragma unroll
        for (int d = 0; d < DFE_AHEAD; d++) {
            const int p = p0 + d;
            if (p >= e) break;
            if (p == s) {
#pragma unroll
                for (int j = 0; j < K2M; j++)
                    if (j < K2) sp[K2 - 1 - j] = (int8_t)st.ix[j];
            }
            const float2 v = q[d];
            q[d] = f[min(p + DFE_AHEAD, e - 1)];
            const int dd = dfe_step<NL, K2M>(v, fr, fi, nfi, st, lev);
            if (p >= s) dr[p] = (int8_t)dd;
        }
    }
}

// Repair pass: one wave per run.  ok[c] = (the speculative pass's decisions at [s_c - K2, s_c) equal chunk c's speculative state), computed
// by all lanes; lane 0 then walks the chunks in order.  A chunk is exact when its start state is: from ok[c] if the walk left the decisions
// in front of s_c untouched, else by comparing the walk's own state registers.  A wrong chunk is re-run from s_c until K2 consecutive new
// decisions inside it equal the old ones (the old ones are then one speculative trajectory with the same state) or the chunk ends.
template <int NL, int K2M>
__global__ __launch_bounds__(64) void dfe_repair_kernel(int N, int K2, int C, int CH, const float2 *__restrict__ ff,
                                                        const float *__restrict__ fb, const float *__restrict__ amp, int8_t *__restrict__ dec,
                                                        const int8_t *__restrict__ spec, int32_t *__restrict__ repairs)
{
    __shared__ uint8_t ok[DFE_CMAX];
    const int run = blockIdx.x, lane = threadIdx.x;
    int8_t *dr = dec + (size_t)run * N;
    const int8_t *sp = spec + (size_t)run * C * DFE_SPEC_B;
    for (int c = 1 + lane; c < C; c += 64) {
        const int s = K2 + c * CH;
        bool eq = true;
        for (int q = 0; q < K2; q++) eq &= dr[s - K2 + q] == sp[(size_t)c * DFE_SPEC_B + q];
        ok[c] = eq;
    }
    __syncthreads();
    if (lane != 0) return;
    float fr[K2M], fi[K2M], nfi[K2M], lev[NL];
    dfe_setup<NL, K2M>(fb + (size_t)run * 2 * K2, amp, K2, fr, fi, nfi, lev);
    const float2 *f = ff + (size_t)run * N;
    DfeState<K2M> st;
    int fixed = 0;
    bool in_regs = false;                                      // the walk re-ran the previous chunk to its end: st is the true state at s_c
    for (int c = 1; c < C; c++) {
        const int s = K2 + c * CH, e = min(N, s + CH);
        bool exact;
        if (in_regs) {
            exact = true;
#pragma unroll
            for (int j = 0; j < K2M; j++)
                if (j < K2) exact &= st.ix[j] == (int)sp[(size_t)c * DFE_SPEC_B + K2 - 1 - j];
        } else {
            exact = ok[c];
        }
        if (exact) {
            in_regs = false;
            continue;
        }
        if (!in_regs) dfe_load_state<NL, K2M>(st, dr, s, K2, amp);
        int p = s, match = 0;
        float2 v = f[p];
        while (p < e) {
            const float2 vn = f[min(p + 1, e - 1)];
            const int old = (uint8_t)dr[p];
            const int d = dfe_step<NL, K2M>(v, fr, fi, nfi, st, lev);
            dr[p] = (int8_t)d;
            p++;
            v = vn;
            match = d == old ? match + 1 : 0;
            if (match >= K2) break;
        }
        fixed += p - s;
        in_regs = p == e;
    }
    if (repairs) repairs[run] = fixed;
}

// find_shift_symb(hard decisions, data, n_shift) and SER_func(hard[:, n_cut+11+shift : -11-n_cut], data[:, n_cut+11 : -11-shift-n_cut])
// (:290-293); the hard-decision track is const_torch[dec] = (lev[dec / n], lev[dec % n]).
__global__ __launch_bounds__(LE_NT) void dfe_eval_kernel(int N, int n_lev, int n_shift, int n_cut, const int8_t *__restrict__ dec,
                                                         const float *__restrict__ amp, const __half *__restrict__ data,
                                                         float *__restrict__ ser, int32_t *__restrict__ shift_out)
{
    __shared__ float red[LE_NT / 64];
    __shared__ float corr[2][64];
    __shared__ float lev[8];
    __shared__ int sh_shift;
    const int run = blockIdx.x, tid = threadIdx.x;
    if (tid < n_lev) lev[tid] = amp[tid];
    __syncthreads();
    const int8_t *dr = dec + (size_t)run * N;
    auto trk = [&](int m) {
        const int d = (uint8_t)dr[m];                          // < n_lev^2 (masked all the same: the lookups stay inside lev)
        return make_float2(lev[(d / n_lev) % n_lev], lev[d % n_lev]);
    };
    const __half *tx0 = data + (size_t)run * 2 * N, *tx1 = tx0 + N;
    const int shift = eval_find_shift<LE_NT>(trk, tx0, tx1, n_shift, N, corr, &sh_shift, tid);
    const int L = N - 22 - 2 * n_cut - shift;
    const float s = eval_ser<LE_NT>(trk, n_cut + 11 + shift, L, tx0 + n_cut + 11, tx1 + n_cut + 11, L, lev, n_lev, red, tid);
    if (tid == 0) {
        ser[run] = s;
        if (shift_out) shift_out[run] = shift;
    }
}

template <int NL, int K2M>
static void launch_dfe_recursion(hipStream_t st, int R, int N, int K2, int C, int CH, int W, const float2 *ff, const float *fb,
                                 const float *amp, const int8_t *init, int8_t *dec, int8_t *spec, int32_t *repairs)
{
    hipLaunchKernelGGL((dfe_spec_kernel<NL, K2M>), dim3((R * C + 255) / 256), dim3(256), 0, st, R, N, K2, C, CH, W, ff, fb, amp, init, dec, spec);
    hipLaunchKernelGGL((dfe_repair_kernel<NL, K2M>), dim3(R), dim3(64), 0, st, N, K2, C, CH, ff, fb, amp, dec, spec, repairs);
    note_kernel("vaeq::dfe_repair_kernel<%d, %d>", NL, K2M);   // the spec kernel carries the same template arguments
}

}  // namespace vaeq

// Shared shape rules of both entry points: sps == 1 (the script's only setting), n_lev in {2, 4, 8}, the shift search inside the first 1000
// symbols and the evaluation slices non-empty.
static bool awgn_genie_shape(int32_t R, int64_t N, int32_t sps, int32_t n_lev, int32_t K, int32_t n_shift, int32_t n_cut, bool eval = true)
{
    if (R < 0 || N <= 0 || N > (1 << 30) || sps != 1 || !(n_lev == 2 || n_lev == 4 || n_lev == 8) || K < 1 || K > vaeq::DFE_KMAX) return false;
    return !eval || (n_shift >= 1 && n_shift <= 64 && n_cut >= 0 && n_shift / 2 <= n_cut + 11 && N >= 1000 + n_shift + 2 * n_cut + 22);
}

extern "C" int64_t vaeq_awgn_lmmse_eval_ws_bytes(int32_t R, int64_t N, int32_t K)
{
    if (R < 0 || N <= 0 || K < 1 || K > vaeq::DFE_KMAX) return VAEQ_ERR_SHAPE;
    return (int64_t)R * (N + 2 * (K / 2) - K + 1) * (int64_t)sizeof(float2);
}

extern "C" int vaeq_awgn_lmmse_eval(int32_t R, int64_t N, int32_t sps, int32_t n_lev, int32_t K, int32_t n_shift, int32_t n_cut,
                                    const float *rx, const float *taps, const float *amp, const void *data_f16, float *ws, float *ser,
                                    int32_t *shift, int8_t *dec, float *out, void *stream)
{
    if (!awgn_genie_shape(R, N, sps, n_lev, K, n_shift, n_cut) || (K & 1)) return VAEQ_ERR_SHAPE;
    if (R == 0) return VAEQ_OK;
    if (!rx || !taps || !amp || !data_f16 || !ser || (!out && !ws)) return VAEQ_ERR_NULL;
    float2 *track = reinterpret_cast<float2 *>(out ? out : ws);
    return vaeq::launch(vaeq::lmmse_eval_kernel, dim3(R), dim3(vaeq::LE_NT), 0, reinterpret_cast<hipStream_t>(stream), (int)N, K, n_lev, n_shift,
                        n_cut, rx, taps, amp, reinterpret_cast<const __half *>(data_f16), track, dec, ser, shift);
}

// Chunks of the speculative pass: CH = ceil((N - K2) / C) symbols, C reduced to the number of non-empty chunks.
static int32_t dfe_chunk_len(int64_t N, int32_t K2, int32_t C) { return (int32_t)((N - K2 + C - 1) / C); }

static bool dfe_shape(int32_t R, int64_t N, int32_t K2, int32_t C, int32_t W)
{
    if (K2 < 1 || K2 > 10 || C < 1 || C > vaeq::DFE_CMAX || W < 0 || N - K2 < C) return false;
    return C == 1 || dfe_chunk_len(N, K2, C) >= K2;           // the repair walk reads a chunk's start state from the chunk before it alone
}

extern "C" int64_t vaeq_awgn_dfe_ws_bytes(int32_t R, int64_t N, int32_t C)
{
    if (R < 0 || N <= 0 || C < 1 || C > vaeq::DFE_CMAX) return VAEQ_ERR_SHAPE;
    return (int64_t)R * N * (int64_t)sizeof(float2) + (int64_t)R * C * vaeq::DFE_SPEC_B;
}

extern "C" int vaeq_awgn_dfe(int32_t R, int64_t N, int32_t sps, int32_t n_lev, int32_t K1, int32_t K2, int32_t C, int32_t W, int32_t n_shift,
                             int32_t n_cut, const float *rx, const float *ff_taps, const float *fb_taps, const float *amp, const int8_t *init_dec,
                             const void *data_f16, void *ws, int8_t *dec, float *ser, int32_t *shift, int32_t *repairs, float *ff_out,
                             void *stream)
{
    if (!awgn_genie_shape(R, N, sps, n_lev, K1, n_shift, n_cut, ser != nullptr) || !dfe_shape(R, N, K2, C, W)) return VAEQ_ERR_SHAPE;
    if (R == 0) return VAEQ_OK;
    if (!rx || !ff_taps || !fb_taps || !amp || !init_dec || !ws || !dec || (ser && !data_f16)) return VAEQ_ERR_NULL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int CH = dfe_chunk_len(N, K2, C);
    C = (int32_t)((N - K2 + CH - 1) / CH);
    float2 *ff = ff_out ? reinterpret_cast<float2 *>(ff_out) : reinterpret_cast<float2 *>(ws);
    int8_t *spec = reinterpret_cast<int8_t *>(ws) + (size_t)R * N * sizeof(float2);
    hipLaunchKernelGGL(vaeq::dfe_ff_kernel, dim3((unsigned)((N + 255) / 256), R), dim3(256), 0, st, (int)N, K1, rx, ff_taps, ff);
    const int n = (int)N;
    vaeq::dispatch_nlev(n_lev, [&](auto nl) {                  // (n_lev was checked above; a chain of launches reports its status once, below)
        constexpr int NL = decltype(nl)::value;
        if (K2 <= 4) vaeq::launch_dfe_recursion<NL, 4>(st, R, n, K2, C, CH, W, ff, fb_taps, amp, init_dec, dec, spec, repairs);
        else vaeq::launch_dfe_recursion<NL, 10>(st, R, n, K2, C, CH, W, ff, fb_taps, amp, init_dec, dec, spec, repairs);
        return (int)VAEQ_OK;
    });
    if (ser)
        hipLaunchKernelGGL(vaeq::dfe_eval_kernel, dim3(R), dim3(vaeq::LE_NT), 0, st, n, n_lev, n_shift, n_cut, dec, amp,
                           reinterpret_cast<const __half *>(data_f16), ser, shift);
    return hipGetLastError() == hipSuccess ? VAEQ_OK : VAEQ_ERR_LAUNCH;
}
