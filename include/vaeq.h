/*
 * vaeq.h -- C ABI of libvaeq_hip.so: the MI355X (gfx950) implementation of the
 * VAE blind-equalizer training inner loop of kit-cel/vae-equalizer.
 *
 * The reference has no FFI: its "operator interface" for this path is a set of
 * Python callables.  Each entry point below names the
 * reference code it replaces (paths relative to the reference tree) and is what
 * a binding of that code would call; INTEGRATION.md shows the ctypes stubs.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer to row-major fp32 unless noted;
 *   - the caller owns all buffers; kernels keep no state between calls
 *     (equalizer taps, channel estimate, Adam moments and step counters are
 *     caller-owned arrays that are updated in place);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls
 *     are asynchronous with respect to the host;
 *   - return value: 0 = ok, negative = error (vaeq_strerror), never throws;
 *   - one "run" = one independent Monte-Carlo run / sweep point
 *     (optical_DP_channel/Eval_run_DP.py:68-86); runs never communicate.
 */
#ifndef VAEQ_H
#define VAEQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAEQ_VERSION 100

enum {
    VAEQ_OK = 0,             /* also for an empty batch (R == 0): nothing is read, pointers may be NULL */
    VAEQ_ERR_NULL = -1,      /* a required pointer is NULL */
    VAEQ_ERR_SHAPE = -2,     /* inconsistent or unsupported sizes (even M, n_lev not in {2,4,8}, window past S ...) */
    VAEQ_ERR_LDS = -3,       /* the per-run working set does not fit the 160 KiB LDS of a CU */
    VAEQ_ERR_LAUNCH = -4,    /* HIP launch error (hipGetLastError) */
    VAEQ_ERR_DEVICE = -5     /* not a gfx950 device / no device */
};

/* ------------------------------------------------------------------------
 * Dual-polarisation VAE-LE / VAEflex training loop.
 *
 * Replaces, for R independent runs at once, the minibatch loop
 *   optical_DP_channel/func_VAELE_DP_MQAM_shaping.py:57-66   (VAE-LE)
 *   optical_DP_channel/func_VAEflex_DP_MQAM_shaping.py:59-70 (VAEflex)
 * i.e. per step: twoXtwoFIR.forward (shared_funcs.py:500-527), loss_function_shaping
 * (shared_funcs.py:92-137), loss.backward(), optim.Adam.step() for both parameter
 * groups (func_VAELE_DP_MQAM_shaping.py:28,31), and the copies into
 * out_train / out_const / var_est (:61-62,64).
 *
 * Window of step s of frame f starts at symbol s*stride_sym of that frame's row
 * and spans B symbols (= B*sps samples, zero-padded by M/2 samples on both sides
 * exactly like Conv1d(padding=M//2), shared_funcs.py:494).
 *   VAE-LE : stride_sym = B,         keep_off = 0,               keep_len = B
 *   VAEflex: stride_sym = flex_step, keep_off = (B-flex_step)/2, keep_len = flex_step
 */
typedef struct vaeq_dp_args {
    int32_t R;           /* independent runs in this call (one workgroup each) */
    int32_t n_frames;    /* frames per run held in rx (taps/Adam state carry across frames; a launch of up to 16 frames is bit-identical to
                            the same frames launched one by one: the Adam bias corrections restart at every frame head as at a launch) */
    int32_t steps;       /* minibatch steps per frame */
    int32_t B;           /* batch_len: symbols per minibatch window */
    int32_t sps;         /* samples per symbol (reference: 2) */
    int32_t M;           /* M_est: taps of the butterfly FIR and of h_est; odd, <= 63 */
    int32_t n_lev;       /* ASK levels per axis: 2, 4 or 8 (4-/16-/64-QAM) */
    int32_t stride_sym;  /* symbols between consecutive window starts */
    int32_t keep_off;    /* first window-local symbol copied to q_out / y_out */
    int32_t keep_len;    /* number of window-local symbols copied per step */
    int64_t S;           /* samples per (run, frame, pol, I/Q) row of rx */
    const float *rx;     /* [R][n_frames][2 pol][2 I/Q][S]   received samples (rx_tensor, shared_funcs.py:88) */
    float *W;            /* [R][2][4][M]     FIR weight, nn.Conv1d(4,2,M) layout (shared_funcs.py:494) */
    float *h;            /* [R][2][2][2][M]  h_est[chi][nu][re/im][tap] (shared_funcs.py:583-586) */
    float *adam_mW, *adam_vW;   /* [R][2][4][M]     exp_avg / exp_avg_sq of W */
    float *adam_mh, *adam_vh;   /* [R][2][2][2][M]  exp_avg / exp_avg_sq of h */
    int32_t *step;       /* [R] Adam step count (in: steps done so far; out: += n_frames*steps) */
    const float *amp;    /* [n_lev]    amp_levels, shared by all runs (shared_funcs.py:568) */
    const float *P;      /* [R][n_lev] PCS pmf of the levels (shared_funcs.py:572) */
    const float *var;    /* [R][2]     demapper noise variance per polarisation (shared_funcs.py:581) */
    const float *nu_sc;  /* [R]        rescaled shaping factor (shared_funcs.py:570) */
    const float *lr_W;   /* [R] learning rate of param group 0 (W) for this call (func_VAELE_DP...:45-46) */
    const float *lr_h;   /* [R] learning rate of param group 1 (h_est) */
    float *q_out;        /* nullable [R][n_frames][2][2*n_lev][steps*keep_len]  out_train */
    float *y_out;        /* nullable [R][n_frames][2][2][steps*keep_len]        out_const */
    float *loss;         /* nullable [R][n_frames][steps]                        ELBO per minibatch */
    float *var_est;      /* nullable [R][n_frames][2][steps]                     C/(N-Mh) per minibatch */
    float *eq_out;       /* nullable [R][n_frames][2][steps*keep_len]   E_q[x_I] per polarisation: all find_shift reads of q
                            (shared_funcs.py:296-297) */
    int8_t *dec_out;     /* nullable [R][n_frames][2][2][steps*keep_len] argmax_i q_i per axis: all SER_IQflip reads of q (:201).
                            With eq_out + dec_out the per-frame epilogue needs no q: q_out may be NULL (32 of the 44 floats a
                            DP symbol costs in HBM are the materialised q) */
    float *dbg_gW;       /* nullable [R][2][4][M]     gradient of the LAST step (parity tests) */
    float *dbg_gh;       /* nullable [R][2][2][2][M] */
    int32_t threads;     /* kernel choice: 0 = automatic: the wave-per-run fast path when the shape allows (sps = 2, B <= 1024 even or
                            odd, M one of 9 13 17 21 25 31), else the generic kernel with 256 threads per run.
                            1 = wave-per-run only (VAEQ_ERR_SHAPE if unsupported); 64 / 128 / 256 = generic kernel, that
                            many threads per run */
    int32_t no_update;   /* 1: skip the Adam update (forward + loss + gradients only) */
} vaeq_dp_args;

int vaeq_dp_train(const vaeq_dp_args *args, void *stream);

/* SURVEY 8(b)'s `vaeq_dp_step_debug`: ONE minibatch step per run that additionally dumps the step's gradients, for teacher-forced parity
 * tests against loss.backward() of the reference (func_VAELE_DP_MQAM_shaping.py:64-65: dL/dW as net.conv_w.weight.grad [2][4][M], dL/dh_est
 * [2][2][2][M]).  = vaeq_dp_train on the first window of the first frame (n_frames and steps taken as 1) with dbg_gW / dbg_gh pointed at
 * gW / gh; args->no_update chooses between "gradients only" and "gradients + the Adam step"; every other field as for vaeq_dp_train.
 * (vaeq_dp_train itself dumps the LAST step's gradients when args->dbg_gW / dbg_gh are set: same kernels, same values.) */
int vaeq_dp_step_debug(const vaeq_dp_args *args, float *gW, float *gh, void *stream);

/* LDS bytes one run (= one workgroup) needs for the given shape, or a negative error code. */
int64_t vaeq_dp_lds_bytes(int32_t B, int32_t sps, int32_t M, int32_t n_lev);

/* How many runs of this shape the current device keeps co-resident (occupancy x compute units) with the kernel that
 * `threads` selects (same meaning as vaeq_dp_args.threads; VAE-LE geometry assumed).  Sweeps sized to a multiple of it
 * have no partially filled last round.  Negative error code on failure. */
int64_t vaeq_dp_resident_runs(int32_t B, int32_t sps, int32_t M, int32_t n_lev, int32_t threads);

/* ------------------------------------------------------------------------
 * Stand-alone soft demapper:  shared_funcs.py:529-542 (soft_dec), the same
 * formula as the demapping half of twoXtwoFIR.forward (shared_funcs.py:521-523).
 * y[R][2][2][N] -> q[R][2][2*n_lev][N];  amp[n_lev]; var[R][2]; nu_sc[R].
 */
int vaeq_soft_demap(int32_t R, int64_t N, int32_t n_lev, const float *y, const float *amp, const float *var,
                    const float *nu_sc, float *q, void *stream);

/* ------------------------------------------------------------------------
 * Butterfly FIR + soft demapper without training (twoXtwoFIR.forward in eval
 * mode, shared_funcs.py:500-527) on one zero-padded block of N symbols per run:
 * x[R][2][2][N*sps], W[R][2][4][M] -> q[R][2][2*n_lev][N] (nullable), y[R][2][2][N].
 */
int vaeq_dp_forward(int32_t R, int64_t N, int32_t sps, int32_t M, int32_t n_lev, const float *x, const float *W,
                    const float *amp, const float *var, const float *nu_sc, float *q, float *y, void *stream);

/* ------------------------------------------------------------------------
 * ELBO of one minibatch per run, values only: shared_funcs.py:92-137 (loss_function_shaping).
 * q[R][2][2*n_lev][B], x[R][2][2][B*sps], h[R][2][2][2][M], P[R][n_lev] -> loss[R], var_est[R][2].
 */
int vaeq_dp_loss(int32_t R, int32_t B, int32_t sps, int32_t M, int32_t n_lev, const float *q, const float *x,
                 const float *h, const float *amp, const float *P, float *loss, float *var_est, void *stream);

/* ------------------------------------------------------------------------
 * Backward passes of the two stand-alone operators (for torch.autograd.Function wrappers: a reference-style
 * `loss.backward(); optimizer.step()` loop on HIP kernels; the fused vaeq_dp_train does not use them).
 *   vaeq_dp_loss_bwd   : loss_function_shaping (shared_funcs.py:92-137): g_up[R] = upstream d/dloss ->
 *                        gq[R][2][2*n_lev][B] = dL/dq, gh[R][2][2][2][M] = dL/dh_est
 *   vaeq_dp_forward_bwd: twoXtwoFIR.forward (shared_funcs.py:500-527): gq = dL/dq, gy = dL/dout (nullable), with the forward's
 *                        q, y -> gW[R][2][4][M] = dL/dW (softmin backward, then the conv weight gradient)
 */
int vaeq_dp_loss_bwd(int32_t R, int32_t B, int32_t sps, int32_t M, int32_t n_lev, const float *q, const float *x, const float *h,
                     const float *amp, const float *P, const float *g_up, float *gq, float *gh, void *stream);
int vaeq_dp_forward_bwd(int32_t R, int32_t N, int32_t sps, int32_t M, int32_t n_lev, const float *x, const float *q, const float *y,
                        const float *gq, const float *gy, const float *amp, const float *var, float *gW, void *stream);

/* Input gradients of the same two operators (complex gradients packed as d/dRe + j d/dIm, like x itself); fixed summation order, no atomics.
 *   vaeq_dp_loss_bwd_x   : loss_function_shaping (shared_funcs.py:123-129: rx enters through e = rx[mh:-mh] - D): g_up[R] ->
 *                          gx[R][2][2][B*sps] = dL/drx = g_up (nm / C_chi) 2 e on the nm inner samples, exactly 0 on the mh samples at either end
 *   vaeq_dp_forward_bwd_x: twoXtwoFIR.forward (shared_funcs.py:500-516, the two strided Conv1d over the packed input): gq, gy (nullable), the
 *                          forward's q, y and the taps W[R][2][4][M] -> gx[R][2][2][N*sps] = dL/dx, the transposed strided correlation
 *                          gx[p][s] = sum_o sum_{n sps + k - M/2 = s} conj(w[o][p][k]) dL/dout[o][n]  (dL/dout as vaeq_dp_forward_bwd forms it)
 * Ceilings: vaeq_dp_loss_bwd's for the loss; 4 (4 N + 8 M) bytes of LDS for the FIR. */
int vaeq_dp_loss_bwd_x(int32_t R, int32_t B, int32_t sps, int32_t M, int32_t n_lev, const float *q, const float *x, const float *h,
                       const float *amp, const float *g_up, float *gx, void *stream);
int vaeq_dp_forward_bwd_x(int32_t R, int32_t N, int32_t sps, int32_t M, int32_t n_lev, const float *W, const float *q, const float *y,
                          const float *gq, const float *gy, const float *amp, const float *var, float *gx, void *stream);

/* ------------------------------------------------------------------------
 * Single-polarisation (AWGN / ISI channel) VAE-LE training loop.
 *
 * Replaces, for R independent runs at once, the minibatch loop
 *   AWGN_channel/func_VAELE_MQAM_shaping.py:297-306
 * i.e. per step: twoFIR.forward (:214-231, with the mean-|y| normalisation), loss_function (:63-95),
 * loss.backward(), optim.Adam(amsgrad=True).step() for both parameter groups (:283-286).
 * Minibatches are contiguous and non-overlapping: step s uses symbols [s*B, (s+1)*B) of the row.
 */
typedef struct vaeq_awgn_args {
    int32_t R;           /* independent runs (one workgroup each) */
    int32_t steps;       /* minibatch steps in this call (N_train // batch_len per epoch, :297) */
    int32_t B;           /* batch_len */
    int32_t sps;         /* samples per symbol */
    int32_t M;           /* M_est: taps of the FIR and of h_est; odd, <= 63 */
    int32_t n_lev;       /* ASK levels per axis: 2, 4 or 8 */
    int64_t S;           /* samples per (run, I/Q) row of rx */
    const float *rx;     /* [R][2 I/Q][S]  (rx_tensor, :58) */
    float *W;            /* [R][1][2][M]   nn.Conv1d(2,1,M) weight (:209) */
    float *h;            /* [R][2][M]      h_est re/im (:278-280) */
    float *adam_mW, *adam_vW, *adam_xW;   /* [R][2][M] exp_avg, exp_avg_sq, max_exp_avg_sq of W */
    float *adam_mh, *adam_vh, *adam_xh;   /* [R][2][M] ... of h */
    int32_t *step;       /* [R] Adam step count */
    const float *amp;    /* [n_lev]    amp_levels (:260) */
    const float *P;      /* [R][n_lev] pmf of the levels (:264) */
    const float *amp_mean; /* [R]      mean |Re|,|Im| of the shaped constellation (:271) */
    const float *var;    /* [R]        demapper variance 10^(-SNR/10) (:272) */
    const float *lr;     /* [R]        learning rate (both groups, no schedule) */
    float *q_out;        /* nullable [R][2*n_lev][steps*B] */
    float *y_out;        /* nullable [R][2][steps*B]  un-normalised FIR output (:227,231) */
    float *loss;         /* nullable [R][steps] */
    float *dbg_gW;       /* nullable [R][2][M] gradient of the LAST step */
    float *dbg_gh;       /* nullable [R][2][M] */
    int32_t threads;     /* 0 = default, else 64 / 128 / 256 */
    int32_t no_update;   /* 1: skip the Adam update */
} vaeq_awgn_args;

int vaeq_awgn_train(const vaeq_awgn_args *args, void *stream);
int64_t vaeq_awgn_lds_bytes(int32_t B, int32_t sps, int32_t M, int32_t n_lev);

/* Stand-alone ELBO of the single-polarisation variants for a given q (values): func_VAELE_MQAM_shaping.loss_function (:63-95) with
 * P[R][n_lev], func_VAENN_MQAM.loss_function (:63-95, entropy instead of KL) with P == NULL.
 * q[R][2*n_lev][B], x[R][2][B*sps], h[R][2][M] -> loss[R]. */
int vaeq_awgn_loss(int32_t R, int32_t B, int32_t sps, int32_t M, int32_t n_lev, const float *q, const float *x, const float *h,
                   const float *amp, const float *P, float *loss, void *stream);

/* Backward passes of the two stand-alone AWGN operators (for autograd wrappers, like vaeq_dp_loss_bwd / vaeq_dp_forward_bwd):
 *   vaeq_awgn_loss_bwd   : g_up[R] -> gq[R][2*n_lev][B] = dL/dq, gh[R][2][M] = dL/dh   (P nullable as in vaeq_awgn_loss)
 *   vaeq_awgn_forward_bwd: twoFIR.forward (:214-231): gq[R][2*n_lev][N] (+ nullable gy[R][2][N] on the un-normalised output)
 *                          -> gW[R][2][M]; the forward is recomputed from x and W. */
int vaeq_awgn_loss_bwd(int32_t R, int32_t B, int32_t sps, int32_t M, int32_t n_lev, const float *q, const float *x, const float *h,
                       const float *amp, const float *P, const float *g_up, float *gq, float *gh, void *stream);
int vaeq_awgn_forward_bwd(int32_t R, int32_t N, int32_t sps, int32_t M, int32_t n_lev, const float *x, const float *W, const float *amp,
                          const float *amp_mean, const float *var, const float *gq, const float *gy, float *gW, void *stream);

/* Input gradients of the two stand-alone AWGN operators:
 *   vaeq_awgn_loss_bwd_x   : loss_function (func_VAELE_MQAM_shaping.py:84-89 / func_VAENN_MQAM.py:84-89; the prior plays no part): g_up[R] ->
 *                            gx[R][2][B*sps] = g_up (nm / C) 2 e on the inner samples, exactly 0 on the M/2 samples at either end
 *   vaeq_awgn_forward_bwd_x: twoFIR.forward (func_VAELE_MQAM_shaping.py:214-231): gq (+ nullable gy on the un-normalised output) ->
 *                            gx[R][2][N*sps]; dL/dout includes the normalisation's Jacobian (:228) as in vaeq_awgn_forward_bwd, then the
 *                            transposed strided correlation with w = W0 - j W1.  Same LDS ceilings as the two siblings. */
int vaeq_awgn_loss_bwd_x(int32_t R, int32_t B, int32_t sps, int32_t M, int32_t n_lev, const float *q, const float *x, const float *h,
                         const float *amp, const float *g_up, float *gx, void *stream);
int vaeq_awgn_forward_bwd_x(int32_t R, int32_t N, int32_t sps, int32_t M, int32_t n_lev, const float *x, const float *W, const float *amp,
                            const float *amp_mean, const float *var, const float *gq, const float *gy, float *gx, void *stream);

/* twoFIR.forward in eval mode (validation pass, func_VAELE_MQAM_shaping.py:311-313) on N symbols per run:
 * x[R][2][N*sps], W[R][2][M] -> q[R][2*n_lev][N] (nullable), y[R][2][N] (un-normalised). */
int vaeq_awgn_forward(int32_t R, int64_t N, int32_t sps, int32_t M, int32_t n_lev, const float *x, const float *W,
                      const float *amp, const float *amp_mean, const float *var, float *q, float *y, void *stream);

/* ------------------------------------------------------------------------
 * Per-frame epilogue of the DP runs: shift / polarisation-swap search and both SER estimators,
 *   shared_funcs.py:188-338 with the roll / cut / slice logic of func_VAELE_DP_MQAM_shaping.py:68-89 (batch_len > 0)
 *   or func_VAEflex_DP_MQAM_shaping.py:72-84 (batch_len = 0: no per-minibatch cut).
 * q[R][2][2*n_lev][N] (out_train), y[R][2][2][N] (out_const), tx_f16[R][2][2][N] IEEE half (data_tensor, shared_funcs.py:89),
 * var[R][2], nu_sc[R] -> ser[R][4] (rows: constellation x, y; soft demapper x, y), shift[R][2 path][2] (path 0 = q, 1 = y),
 * rflag[R][2].  workspace: vaeq_dp_epilogue_ws_bytes(R, N) bytes of device memory.
 * The cuts are Python slices, as in the reference.  Of every minibatch [: batch_len - shift[0] - 10] is kept: all of it when that end is
 * >= batch_len, nothing when it is 0, and batch_len + end symbols when it is NEGATIVE (batch_len < shift[0] + 10, so only for batch_len < 20),
 * since a negative end counts from the minibatch's end.  Of the (N / batch_len) * kept symbols that remain, [11 : -11 - max|shift|] is kept.
 * A path whose window is empty (N >= 43 does not exclude that when batch_len > 0) reports NaN in its two ser rows -- the mean of an
 * empty slice -- never 0. */
int vaeq_dp_epilogue(int32_t R, int64_t N, int32_t n_lev, int32_t batch_len, const float *q, const float *y, const void *tx_f16,
                     const float *amp, const float *var, const float *nu_sc, float *ser, int32_t *shift, int32_t *rflag,
                     void *workspace, void *stream);
int64_t vaeq_dp_epilogue_ws_bytes(int32_t R, int64_t N);
/* Same epilogue fed by the training kernel's compact outputs instead of q: eq[R][2][N] (vaeq_dp_args.eq_out) and dec[R][2][2][N]
 * (dec_out) of ONE frame; results are bit-identical to vaeq_dp_epilogue on the q of the same call. */
int vaeq_dp_epilogue_compact(int32_t R, int64_t N, int32_t n_lev, int32_t batch_len, const float *eq, const int8_t *dec, const float *y,
                             const void *tx_f16, const float *amp, const float *var, const float *nu_sc, float *ser, int32_t *shift,
                             int32_t *r_flag, void *stream);

/* Information-rate figures of one DP frame, per run and polarisation, over exactly the symbols the soft-demapper SER of vaeq_dp_epilogue keeps
 * (shift[R][2] / rflag[R] = that call's path-0 alignment: the same roll, polarisation exchange, per-minibatch cut and frame-edge slice).
 * Exactly one of q[R][2][2*n_lev][N] (posteriors as stored) and y[R][2][2][N] (equalised samples; the posteriors are recomputed by the soft
 * demapper's formula with var[R][2] / nu_sc[R], in the log domain -- the form for the compact pipeline, which never materialises q) is given;
 * var and nu_sc may be NULL with q.  tx_f16[R][2][2][N] IEEE half, amp[n_lev], P[R][n_lev] the runs' per-axis pmf.
 * Level i carries the binary-reflected Gray label g(i) = i ^ (i >> 1), b = log2 n_lev bits per axis; H = -sum P log2 P.  Of the eight
 * hypotheses h = 4 flip + rot (rot: 0, pi, pi/2, 3 pi/2; shared_funcs.py:188-222) the one with the fewest symbol errors of argmax(q) wins, ties
 * to the smallest h, so sym_err / kept IS the soft-demapper SER.  Under it, with l(x) = log2 max(x, FLT_MIN) (y-mode: an exact log-softmax):
 *   AIR = 2 H + mean[l(q_I[t_I]) + l(q_Q[t_Q])]                                   (symbol-wise mismatched decoding, bit per 2-D symbol)
 *   GMI = 2 H + mean sum_axis sum_k l(sum of q_axis[i] over the i whose label bit k equals that of the transmitted level)
 *   BER = bit_err / (2 b kept), bit_err = differing label bits between decided and transmitted level, both axes
 * (NGMI = 1 - (2 H - GMI) / (2 b) is the host's).  info[R][2][3] = AIR, GMI, BER; counts[R][2][4] = kept, sym_err, bit_err, hyp.  An empty
 * window gives NaN figures and zero counts.  q is read once; sums run in a fixed order without float atomics: two calls give identical bits. */
int vaeq_dp_epilogue_info(int32_t R, int64_t N, int32_t n_lev, int32_t batch_len, const float *q, const float *y, const void *tx_f16,
                          const float *amp, const float *P, const float *var, const float *nu_sc, const int32_t *shift,
                          const int32_t *rflag, float *info, int32_t *counts, void *stream);

/* The per-bit a-posteriori LLRs of one DP frame: the input of a bit-wise (LDPC) decoder behind the equaliser, of which the GMI of
 * vaeq_dp_epilogue_info is the rate.  Same sources, alignment and window as that call: exactly one of q[R][2][2*n_lev][N] and y[R][2][2][N]
 * (var[R][2] and nu_sc[R] are required with y and may be NULL with q), amp[n_lev], shift[R][2] / rflag[R] = vaeq_dp_epilogue's path-0
 * alignment, batch_len its per-minibatch cut.  hyp[R][2] = the hypothesis per run and polarisation, counts[..][3] of vaeq_dp_epilogue_info; it
 * is used as hyp & 7 and only selects values, no address depends on it.
 * For one symbol and one received axis c, with L[c][k][s] the log2 of the posterior mass of the levels i whose label bit k of
 * g(i) = i ^ (i >> 1) is s (q-mode: log2 max(sum, FLT_MIN) of the set sums added in ascending i, so an exact 0 costs 126 bit and every LLR is
 * finite; y-mode: a log-sum-exp of each set around its own maximum over the soft demapper's exponent, with the var of the RECEIVED row):
 *   lam[c][k] = ln 2 (L[c][k][0] - L[c][k][1])                  nats, positive = bit 0, a-posteriori (the priors are in the posteriors)
 * Hypothesis h = 4 flip + rot finds the transmitted axes: rot 0: I' = axis 0, Q' = axis 1; pi: both reversed; pi/2: I' = axis 1 reversed,
 * Q' = axis 0; 3 pi/2: I' = axis 1, Q' = axis 0 reversed; the flip reverses Q' once more.  Reversing a level order flips the top label bit only
 * (g(n-1-i) = g(i) ^ n/2): it negates plane k = b-1 of that axis and nothing else (b = log2 n_lev).
 * llr[R][2][2 b][N] float32: plane a b + k of output polarisation p holds bit k of TX axis a (0 = I, 1 = Q), indexed by the TX symbol index n,
 * so the planes line up with tx[R][2][2][N].  It reads sample n + clamp(shift[p], -10, 10) of row (p - r) & 1 and is kept iff the window of
 * vaeq_dp_epilogue_info keeps n and that sample lies in [0, N); every other entry is an erasure, written as +0.0 (the buffer may be
 * uninitialised).  Elementwise, no atomics: two calls give identical bits.
 * R == 0 is VAEQ_OK (its pointers may be NULL); both or neither of q and y is VAEQ_ERR_NULL, before any shape rule; then any other NULL
 * pointer; R < 0, N < 43, N > 0x3fffffff, batch_len < 0, N % batch_len != 0 or n_lev not in {2, 4, 8} is VAEQ_ERR_SHAPE. */
int vaeq_dp_epilogue_llr(int32_t R, int64_t N, int32_t n_lev, int32_t batch_len, const float *q, const float *y, const float *amp,
                         const float *var, const float *nu_sc, const int32_t *shift, const int32_t *rflag, const int32_t *hyp, float *llr,
                         void *stream);

/* vaeq_awgn_validate for rows under its 64 symbols: the same arguments, results and kernel for 23 + n_shift / 2 <= N < 64 (every shift the
 * search can return, at most n_shift / 2, still keeps a symbol); any other N is VAEQ_ERR_SHAPE, every other refusal is vaeq_awgn_validate's.
 * The reference has no lower limit on the validation frame; vaeq_awgn_validate keeps its own. */
int vaeq_awgn_validate_short(int32_t R, int64_t N, int32_t sps, int32_t M, int32_t n_lev, int32_t n_shift, const float *x, const float *W,
                             const float *amp, const float *amp_mean, const float *var, const void *data_f16, float *y_ws, float *ser,
                             int32_t *shift, void *stream);

/* Information-rate figures of one AWGN validation frame, per run, over exactly the symbols the SER_q of vaeq_awgn_validate / vaeq_nn_validate
 * keeps: for shift[r] = sh the kept symbol j in [0, len), len = N - 22 - sh, pairs the posterior (or sample) 11 + sh + j with the TX symbol
 * 11 + j (q[:, 11+sh : -11] against data[:, 11 : -11-sh], func_VAELE_MQAM_shaping.py:318).  The window is empty when 11 + sh <= 0 or len <= 0;
 * no int32 shift takes an index out of [0, N).  One polarisation, four rotation hypotheses, no IQ flip (SER_q, :97-123).
 * Exactly one of q[R][2*n_lev][N] (posteriors as stored: the output of vaeq_nn_forward) and y[R][2][N] (the un-normalised equaliser output the
 * fused validation leaves in y_ws; amp_mean and var are required with it and may be NULL with q) is given.  data_f16[R][2][N] IEEE half,
 * amp[n_lev], P[R][n_lev] the runs' per-axis pmf.
 * Level i carries the binary-reflected Gray label g(i) = i ^ (i >> 1), S = n_lev - 1, b = log2 n_lev bits per axis; H = -sum P log2 P (a zero
 * entry contributes 0).  TX level t = clamp(rint(S/2 tx + S/2), 0, S) per axis; the decision d_c is the first maximum of the posterior of axis c.
 * Hypothesis h in {0, 1, 2, 3} = rotation by 0, pi, pi/2, 3 pi/2 maps (d_I, d_Q) to (d_I, d_Q), (S - d_I, S - d_Q), (S - d_Q, d_I),
 * (d_Q, S - d_I), the posterior vectors likewise; the one with the fewest symbol errors wins, ties to the smallest h.  Under it, with
 * l(x) = log2 max(x, FLT_MIN) in q-mode and an exact log-softmax in y-mode:
 *   AIR = 2 H + mean[l(q_I'[t_I]) + l(q_Q'[t_Q])]                                 (symbol-wise mismatched decoding, bit per 2-D symbol)
 *   GMI = 2 H + mean sum_axis sum_k l(sum of q_axis'[i] over the i whose label bit k equals that of the transmitted level)
 *   BER = bit_err / (2 b kept), bit_err = sum popcount(g(d') ^ g(t)) over both axes
 * (NGMI = 1 - (2 H - GMI) / (2 b) is the host's).  y-mode posteriors (:228-229): m_c = (sum_{n < N} |y_c[n]|) / N over the WHOLE row,
 * yhat_c = y_c (amp_mean / m_c), z_i = -(yhat_c - a_i)^2 / var, posteriors = log-softmax of z; every bit-wise sum is a log-sum-exp around its own
 * maximum, so nothing underflows.  A component with m_c == 0 has no normalisation: that run reports the empty-window result.  y-mode decides
 * with its own sum for m_c, so sym_err / kept is the validation's SER except where a symbol lies within float32 rounding of a threshold.
 * info[R][3] = AIR, GMI, BER; counts[R][4] = kept, sym_err, bit_err, hyp.  An empty window gives NaN figures and zero counts.  One workgroup
 * per run; sums run in a fixed order without atomics: two calls give identical bits.
 * R == 0 is VAEQ_OK (its pointers may be NULL); both or neither of q and y is VAEQ_ERR_NULL, before any shape rule; R < 0, N < 1,
 * N > 0x3fffffff or n_lev not in {2, 4, 8} is VAEQ_ERR_SHAPE. */
int vaeq_awgn_info(int32_t R, int64_t N, int32_t n_lev, const float *q, const float *y, const void *data_f16, const float *amp, const float *P,
                   const float *amp_mean, const float *var, const int32_t *shift, float *info, int32_t *counts, void *stream);

/* The per-bit a-posteriori LLRs of one AWGN validation frame, under the definition of vaeq_dp_epilogue_llr with the four rotation hypotheses of
 * vaeq_awgn_info (hyp[R] = its counts[..][3], used as hyp & 3; no IQ flip) and that call's sources and window: exactly one of q[R][2*n_lev][N]
 * and y[R][2][N] (amp_mean[R] and var[R] are required with y and may be NULL with q), amp[n_lev], shift[R].  For shift[r] = sh the TX index
 * 11 + j, j < len = N - 22 - sh, reads the posterior (or sample) 11 + sh + j; the window is empty when 11 + sh <= 0 or len <= 0 (64-bit: no
 * int32 shift takes an index out of [0, N)).  y-mode posteriors are vaeq_awgn_info's: yhat_c = y_c (amp_mean / m_c), m_c = (sum_{n < N}
 * |y_c[n]|) / N over the WHOLE row, summed in that kernel's order so that the LLRs are those of the posteriors whose GMI it reports;
 * z_i = -(yhat_c - a_i)^2 / var, each bit-wise set a log-sum-exp around its own maximum.
 * llr[R][2 b][N] float32: plane a b + k holds bit k of TX axis a, indexed by the TX symbol index; everything outside [11, 11 + len) is an
 * erasure, written as +0.0, and an empty window or a component with m_c == 0 writes the whole row as zeros (the buffer may be uninitialised).
 * One workgroup per run; no atomics: two calls give identical bits.
 * R == 0 is VAEQ_OK (its pointers may be NULL); both or neither of q and y is VAEQ_ERR_NULL, before any shape rule; then any other NULL
 * pointer; R < 0, N < 1, N > 0x3fffffff or n_lev not in {2, 4, 8} is VAEQ_ERR_SHAPE. */
int vaeq_awgn_llr(int32_t R, int64_t N, int32_t n_lev, const float *q, const float *y, const float *amp, const float *amp_mean,
                  const float *var, const int32_t *shift, const int32_t *hyp, float *llr, void *stream);

/* The two-stage epilogue of the constant-modulus baselines in one launch (optical_DP_channel/func_CMA_DP_MQAM_shaping.py:39-52 after the phase
 * estimation; the CMAbatch / CMAflex modules are identical there): the constellation stage FIRST (find_shift_symb_full on y, roll / cut,
 * SER_constell_shaping), whose mean-radius normalisation stays in the kept window of the aligned output (the reference normalises a slice view in place,
 * shared_funcs.py:242), then soft_dec (:48) on that and the soft-demapper stage (find_shift_symb_full on E_q[x_I], SER_IQflip on argmax q) -- q is never
 * materialised.  y[R][2][2][N]: phase-corrected output cut to [10:-10]; tx_f16[R][2][2][N]: TX reference cut likewise; ser[R][4] = constellation SER of
 * both polarisations, then soft-demapper SER; shift[R][2][2], rflag[R][2]: index 0 = soft-demapper stage (relative to the aligned sequence), 1 =
 * constellation stage; workspace: vaeq_dp_epilogue_ws_bytes(R, N). */
int vaeq_cma_epilogue(int32_t R, int64_t N, int32_t n_lev, const float *y, const void *tx_f16, const float *amp, const float *var,
                      const float *nu_sc, float *ser, int32_t *shift, int32_t *rflag, void *workspace, void *stream);

/* Information-rate figures of one frame of the constant-modulus baselines, per run and polarisation, over exactly the symbols the soft-demapper SER
 * of vaeq_cma_epilogue keeps; the figures, hypotheses, tie-break, Gray labels and output layout are vaeq_dp_epilogue_info's y-mode (info[R][2][3] =
 * AIR, GMI, BER; counts[R][2][4] = kept, sym_err, bit_err, hyp; NGMI is the host's).  y[R][2][2][N], tx_f16[R][2][2][N], var[R][2], nu_sc[R]: what
 * vaeq_cma_epilogue got; amp[n_lev], P[R][n_lev] the runs' per-axis pmf; shift_c[R][2], r_c[R], shift_q[R][2], r_q[R]: that call's constellation-stage
 * and soft-demapper-stage alignment (shift[:, 1], rflag[:, 1], shift[:, 0], rflag[:, 0]); shifts are clamped to +-10.  The epilogue leaves neither
 * the sequence it demapped nor q in memory, so the kernel redoes both stages' addressing from y:
 *   ya[p'][c][m] = y[(p' - r_c) & 1][c][(m + shift_c[p']) mod N]                      (the roll wraps around the frame)
 *   W_c = [11, N - 11 - max|shift_c|),  fac = sum_{p', m in W_c} |tx[p'][:, m]| / sum_{p', m in W_c} |ya[p'][:, m]|   (one factor per run)
 *   yn = ya fac inside W_c, ya outside it          (the reference normalises a slice view in place, shared_funcs.py:242)
 *   posteriors per axis = softmax_i(-(yn - a_i)^2 / (2 var[p']) - nu_sc a_i^2), in the log domain, every bit-wise sum a log-sum-exp around its own maximum
 *   kept symbol n in [11, N - 11 - max|shift_q|) of output polarisation p reads yn[(p - r_q) & 1][:, n + shift_q[p]]
 * fac is this kernel's own sum, not the epilogue's bit for bit, so sym_err / kept is the epilogue's soft-demapper SER except where a sample lies
 * within float32 rounding of a decision threshold.  A run whose sum of |ya| over W_c is zero has no normalisation: NaN figures, zero counts.
 * One launch, one workgroup per run, y and tx read twice, no workspace; sums run in a fixed order without atomics: two calls give identical bits, R runs in one call
 * the bits of R single calls.
 * R == 0 is VAEQ_OK (its pointers may be NULL); any NULL pointer is VAEQ_ERR_NULL, before any shape rule; R < 0, N < 43, N > 0x3fffffff or n_lev
 * not in {2, 4, 8} is VAEQ_ERR_SHAPE. */
int vaeq_cma_epilogue_info(int32_t R, int64_t N, int32_t n_lev, const float *y, const void *tx_f16, const float *amp, const float *P,
                           const float *var, const float *nu_sc, const int32_t *shift_c, const int32_t *r_c, const int32_t *shift_q,
                           const int32_t *r_q, float *info, int32_t *counts, void *stream);

/* The per-bit a-posteriori LLRs of one frame of the constant-modulus baselines, under the definition of vaeq_dp_epilogue_llr (lam, hypotheses,
 * plane order) with the posteriors of vaeq_cma_epilogue_info, term for term: y[R][2][2][N], tx_f16[R][2][2][N] (needed for fac only), amp[n_lev],
 * var[R][2], nu_sc[R], shift_c[R][2], r_c[R], shift_q[R][2], r_q[R] are what that call got; hyp[R][2] = its counts[..][3], used as hyp & 7 (it
 * selects values only, no address depends on it).  Both shifts are clamped to +-10, ya wraps around the frame, fac is summed over W_c and both
 * polarisations in that kernel's order (per thread at stride 256, over the wave's lanes, over the four waves in order) so that the LLRs are those
 * of the posteriors whose GMI it reports, a sample is scaled by fac exactly where its stage-c index lies in W_c, and output polarisation p is
 * demapped with var of the stage-c aligned row (p - r_q) & 1, each bit-wise set a log-sum-exp around its own maximum.
 * llr[R][2][2 b][N] float32, nats, positive = bit 0: plane a b + k of output polarisation p holds bit k of TX axis a (0 = I, 1 = Q), indexed by the
 * TX symbol index n, so the planes line up with tx[R][2][2][N].  Kept are n in [11, N - 11 - max|shift_q|); every other entry is an erasure,
 * written as +0.0, and a run whose sum of |ya| over W_c is zero writes all zeros (the buffer may be uninitialised: every entry is written).
 * One workgroup per run, or per (run, polarisation) for R <= 512, each forming fac for itself; no atomics: two calls give identical bits, R runs
 * in one call the bits of R single calls on either grid.
 * R == 0 is VAEQ_OK (its pointers may be NULL); any NULL pointer is VAEQ_ERR_NULL, before any shape rule; R < 0, N < 43, N > 0x3fffffff or n_lev
 * not in {2, 4, 8} is VAEQ_ERR_SHAPE. */
int vaeq_cma_epilogue_llr(int32_t R, int64_t N, int32_t n_lev, const float *y, const void *tx_f16, const float *amp, const float *var,
                          const float *nu_sc, const int32_t *shift_c, const int32_t *r_c, const int32_t *shift_q, const int32_t *r_q,
                          const int32_t *hyp, float *llr, void *stream);

/* ------------------------------------------------------------------------
 * Seeded on-device DP channel simulator (input producer): optical_DP_channel/shared_funcs.py:65-90 in three stages with
 * the FFT / inverse FFT over Ls done by the caller (hipFFT through torch.fft) between them.  Counter-based RNG (Philox4x32-10):
 * every value is a function of (seed, frame, run, stream, index) only.
 *   vaeq_gen_dp_tx      : PCS draw (cdf[R][n_lev] = cumulative pmf), zero-stuffing, 'valid' FIR with g[Lg] = h_pulse * h_channel
 *                         (complex, interleaved) -> sig[R][2][Ls] complex64 (interleaved), Ls = sps*(N_conv-1)+1 - Lg + 1;
 *                         data_f16 (nullable) [R][2][2][N]: TX reference = symbols ref_offset .. ref_offset+N-1 (:89)
 *   vaeq_gen_dp_disperse: spectrum x H(f) (PMD + rotation theta[r] + IQ phase e_k = exp(-j phiIQ[k])) x CD phase (:38-54), in place;
 *                         fs = symb_rate * sps; scale multiplies the result (1/Ls folds the inverse FFT's normalisation in)
 *   vaeq_gen_dp_finish  : sigma_n from the mean power (:83), complex AWGN (:84), planar rx[R][2][2][sps*N] (:88); power_ws[R] scratch,
 *                         sigma_out[R] nullable
 * Rows of sig are Lrow >= Ls complex samples long; stage 1 zero-fills [Ls, Lrow).  Lrow == Ls reproduces the reference's circular
 * filtering over the exact sequence length; a padded Lrow (a fast FFT length) turns it into linear filtering -- only the few samples
 * within the dispersion's impulse-response length of the frame edges differ. */
int vaeq_gen_dp_tx(int32_t R, int32_t N, int32_t N_conv, int32_t sps, int32_t n_lev, int32_t Lg, int32_t Ls, int32_t Lrow,
                   int32_t ref_offset, const float *amp, const float *cdf, const float *g_complex, uint64_t seed, uint32_t frame,
                   float *sig_complex, void *data_f16, void *stream);
int vaeq_gen_dp_disperse(int32_t R, int32_t Ls, double fs, double tau_cd, double tau_pmd, float e0_re, float e0_im, float e1_re,
                         float e1_im, float scale, const float *theta, float *spec_complex, void *stream);
int vaeq_gen_dp_finish(int32_t R, int32_t N, int32_t sps, int32_t Ls, int32_t Lrow, const float *snr_db, uint64_t seed, uint32_t frame,
                       const float *sig_complex, float *power_ws, float *rx, float *sigma_out, void *stream);

/* One DP frame in ONE call; same arguments as the stage entry points, e_k = exp(-j phiIQ[k]), fs = symb_rate * sps.  sig_ws[R][2][Lrow]
 * complex64 is scratch.  Two implementations of the same model, same Philox words (results agree to transform rounding):
 *   fused   sps == 2 and Lrow = N1 * 1024 with N1 in {4, 5, 8, 10, 16, 20} (the default frame pads to 20 * 1024): three passes over the signal --
 *           pulse shaping + the N1-point outer DFT stage in registers; per (run, k1) one wavefront: 1024-point FFT, fibre matrix, inverse FFT
 *           (rows through LDS, in place); inverse outer stage + noise + planar split.  No hipFFT.  Twiddles and the per-frequency phases of the
 *           fibre live in library-owned device tables, built once per (device, Lrow, fs, tau_cd, tau_pmd) and immutable afterwards.
 *   staged  any other shape (or env VAEQ_GEN_STAGED=1): the three stage kernels around in-place hipFFT transforms, plans cached per (Lrow, R).
 * power_ws: [R][vaeq_gen_dp_power_parts(Lrow)] floats -- for sps == 2 the first pass leaves partial sums of |sig|^2 there and the noise level
 * (:83) is derived from them: the fibre's transfer matrix is unitary at every frequency (:38-54), the dispersed signal has the power of the
 * undispersed one, so no pass over the dispersed signal is spent on it (other sps: the first R floats, filled by a power pass over the
 * first Ls samples of every row, likewise BEFORE the fibre: on a padded row the dispersed signal leaves some energy in the pad). */
int32_t vaeq_gen_dp_power_parts(int32_t Lrow);               /* max(8, 2 * ceil(Lrow / 2048)) */
int vaeq_gen_dp_frame(int32_t R, int32_t N, int32_t N_conv, int32_t sps, int32_t n_lev, int32_t Lg, int32_t Ls, int32_t Lrow,
                      int32_t ref_offset, const float *amp, const float *cdf, const float *g_complex, const float *snr_db,
                      const float *theta, double fs, double tau_cd, double tau_pmd, float e0_re, float e0_im, float e1_re, float e1_im,
                      uint64_t seed, uint32_t frame, float *sig_ws, float *power_ws, float *rx, void *data_f16, float *sigma_out,
                      void *stream);

/* ------------------------------------------------------------------------
 * the AWGN VAE-NN equalizer (AWGN_channel/func_VAENN_MQAM.py).  Net (:170-188) = Conv1d(2, C, k1, pad k1/2) -> ELU ->
 * Conv1d(C, C, k2, pad k2/2, stride sps) -> per-axis softmax, C = 2 n_lev; loss_function (:63-95); Adam(amsgrad=True) on all
 * parameters (:248-253).  One run's parameters are ONE flat vector in the order of net.parameters() followed by h_est:
 *   theta = [fc1.weight C*2*k1 | fc1.bias C | fc2.weight C*C*k2 | fc2.bias C | h_est 2*M],  vaeq_nn_param_count() floats;
 * the Adam vectors (m, v, max v) and dbg_g use the same layout.  Net_BN (:190-211, batch_norm = 1): BatchNorm1d(C) between the ELU
 * and fc2; theta gains [batch1.weight C | batch1.bias C] in front of h_est, and bn_running[R][2][C] = (running_mean, running_var)
 * is caller-owned state updated by every training step (momentum 0.1) and read by the eval-mode entry points.
 * vaeq_nn_train replaces the minibatch loop (:274-285) for R runs: step s uses symbols [s*B, (s+1)*B) of rx[R][2][S]. */
typedef struct vaeq_nn_args {
    int32_t R, steps, B, sps, M, n_lev, k1, k2;
    int64_t S;
    const float *rx;     /* [R][2][S] */
    float *theta;        /* [R][NP] in/out */
    float *adam_m;       /* [R][NP] in/out */
    float *adam_v;       /* [R][NP] in/out */
    float *adam_x;       /* [R][NP] in/out: max_exp_avg_sq */
    int32_t *step;       /* [R] in/out */
    const float *amp;    /* [n_lev] */
    const float *lr;     /* [R] */
    float *loss;         /* nullable [R][steps] */
    float *q_out;        /* nullable [R][2*n_lev][steps*B] */
    float *dbg_g;        /* nullable [R][NP]: gradient of the LAST step */
    int32_t no_update;   /* 1: skip the Adam update (and the running-statistics update) */
    int32_t batch_norm;  /* 0: Net, 1: Net_BN */
    float *bn_running;   /* Net_BN: [R][2][C] in/out */
} vaeq_nn_args;

int vaeq_nn_train(const vaeq_nn_args *args, void *stream);
int64_t vaeq_nn_param_count(int32_t M, int32_t n_lev, int32_t k1, int32_t k2, int32_t batch_norm);
int64_t vaeq_nn_lds_bytes(int32_t B, int32_t sps, int32_t M, int32_t n_lev, int32_t k1, int32_t k2, int32_t batch_norm);
/* Net.forward in eval mode on N symbols per run (:293-295): x[R][2][N*sps], theta[R][NP] -> q[R][2*n_lev][N].
 * bn_running: NULL for Net; [R][2][C] for Net_BN (net.eval(): the running statistics normalise). */
int vaeq_nn_forward(int32_t R, int64_t N, int32_t sps, int32_t M, int32_t n_lev, int32_t k1, int32_t k2, const float *x,
                    const float *theta, const float *bn_running, float *q, void *stream);

/* The VAE-NN encoder as a stand-alone differentiable operator (func_VAENN_MQAM.Net :170-188 / Net_BN :190-211; the kernels behind the torch
 * modules of the same names), batched over R runs.  These calls act on the NETWORK's parameters only (h_est belongs to the loss):
 *   theta_net = [fc1.weight C*2*k1 | fc1.bias C | fc2.weight C*C*k2 | fc2.bias C]  (Net_BN: ... | batch1.weight C | batch1.bias C),  C = 2 n_lev,
 * vaeq_nn_enc_param_count() floats = vaeq_nn_param_count() - 2 M.  x[R][2][L] with any L >= 1, q[R][2 n_lev][N], N = ceil(L / sps).
 * The reference's residual x_res (:183-185) is constant across the levels of an axis and cancels in the softmax; it is left out.
 * vaeq_nn_enc_forward: training == 0, or Net in either mode: the tiled eval forward of vaeq_nn_forward, no length limit (Net_BN normalises with
 *   bn_running[R][2][C] = running_mean | running_var, read only).  Net_BN with training != 0: batch statistics over the L samples (biased
 *   variance, L >= 2); bn_saved[R][2][C] (nullable) receives mean | 1 / std for the backward pass, bn_running (nullable) moves by momentum 0.1
 *   with the unbiased variance.
 * vaeq_nn_enc_backward: q = the forward's output, gq[R][2 n_lev][N] = ANY upstream gradient dL/dq -> g_theta_net[R][NPnet]; x gets no gradient.
 *   bn_stats: Net: ignored; Net_BN training: the forward's bn_saved; Net_BN eval: bn_running.  ELU(fc1(x)) is recomputed, not saved.
 * The training-mode Net_BN forward and every backward keep a run's whole input in LDS, one workgroup per run: VAEQ_ERR_LDS when
 * vaeq_nn_enc_lds_bytes() exceeds 160 KiB.  No atomics: results are bit-reproducible and do not depend on R.
 * vaeq_nn_enc_backward_x: vaeq_nn_enc_backward (the same g_theta_net, bit for bit) plus the input gradient through fc1 (:179 / :201):
 *   gx[R][2][L]: gx[i][s] = sum_c sum_k fc1.weight[c][i][k] dL/d(fc1 output)[c][s - k + k1 / 2]; x_res (:183-185) cancels in the softmax and adds
 *   nothing.  It needs no LDS beyond vaeq_nn_enc_lds_bytes(), which is its ceiling too. */
int64_t vaeq_nn_enc_param_count(int32_t n_lev, int32_t k1, int32_t k2, int32_t batch_norm);
int64_t vaeq_nn_enc_lds_bytes(int64_t L, int32_t sps, int32_t n_lev, int32_t k1, int32_t k2, int32_t batch_norm);
int vaeq_nn_enc_forward(int32_t R, int64_t L, int32_t sps, int32_t n_lev, int32_t k1, int32_t k2, int32_t batch_norm, int32_t training,
                        const float *x, const float *theta_net, float *bn_running, float *bn_saved, float *q, void *stream);
int vaeq_nn_enc_backward(int32_t R, int64_t L, int32_t sps, int32_t n_lev, int32_t k1, int32_t k2, int32_t batch_norm, int32_t training,
                         const float *x, const float *theta_net, const float *q, const float *gq, const float *bn_stats,
                         float *g_theta_net, void *stream);
int vaeq_nn_enc_backward_x(int32_t R, int64_t L, int32_t sps, int32_t n_lev, int32_t k1, int32_t k2, int32_t batch_norm, int32_t training,
                           const float *x, const float *theta_net, const float *q, const float *gq, const float *bn_stats,
                           float *g_theta_net, float *gx, void *stream);

/* The whole VAE-NN validation block (:287-301: eval forward, find_shift :147-166, SER_q :97-123) in one call, q not materialised:
 * x[R][2][N*sps], theta[R][NP], data_f16[R][2][N] -> ser[R], shift[R] (nullable). */
int vaeq_nn_validate(int32_t R, int64_t N, int32_t sps, int32_t M, int32_t n_lev, int32_t k1, int32_t k2, int32_t n_shift, const float *x,
                     const float *theta, const float *bn_running, const float *amp, const void *data_f16, float *ser, int32_t *shift,
                     void *stream);

/* Single-polarisation AWGN / ISI channel of AWGN_channel/func_VAELE_MQAM_shaping.py:39-61 (generate_data) for R runs, same three
 * stages without the dispersion step: g[Lg] = rrc * h_channel; scratch: power_ws [R][ceil(Ls / 2048)] floats, and sig_ws [R][Ls]
 * complex64 only for sps != 2 (for sps == 2 the clean signal stays in registers: frames of up to four 2048-sample tiles in ONE pass, one workgroup per
 * run; longer ones in two -- one pass for the power, one that adds the noise -- with bit-identical results; env VAEQ_AWGN_TWOPASS=1 forces two);
 * rx[R][2][sps*N] (:57), data_f16 (nullable) [R][2][N] = symbols ref_offset .. ref_offset+N-1 (:59), sigma_out[R] nullable.
 * sigma_fixed (nullable [R]): use this noise standard deviation instead of the power-derived one -- the VAE-NN script's model
 * (func_VAENN_MQAM.py:52: sigma_n = sqrt(1/2) / 10^(SNR/20)); snr_db may then be NULL. */
int vaeq_gen_awgn(int32_t R, int32_t N, int32_t N_conv, int32_t sps, int32_t n_lev, int32_t Lg, int32_t Ls, int32_t ref_offset,
                  const float *amp, const float *cdf, const float *g_complex, const float *snr_db, uint64_t seed, uint32_t frame,
                  float *sig_ws, float *power_ws, float *rx, void *data_f16, float *sigma_out, const float *sigma_fixed, void *stream);

/* Fused validation pass of one AWGN epoch (func_VAELE_MQAM_shaping.py:308-318): twoFIR.forward in eval mode on N symbols per run,
 * find_shift (:188-204, n_shift circular lags over the first 1000 symbols) and SER_q (:97-123, argmax decisions, minimum over the
 * four quadrant rotations, 11 symbols trimmed at both ends) without materialising q.
 * x[R][2][N*sps], W[R][2][M], data_f16[R][2][N] -> ser[R], shift[R] (nullable); y_ws[R][2][N] receives the un-normalised output. */
int vaeq_awgn_validate(int32_t R, int64_t N, int32_t sps, int32_t M, int32_t n_lev, int32_t n_shift, const float *x, const float *W,
                       const float *amp, const float *amp_mean, const float *var, const void *data_f16, float *y_ws, float *ser,
                       int32_t *shift, void *stream);

/* The validation frame of an epoch without its round trip through HBM (func_VAELE_MQAM_shaping.py:310 generate_data followed by :311-318): the
 * reference draws N_valid = 15 000 fresh symbols per evaluated epoch, 12.5 x what it trains on, and reads them once.
 * vaeq_gen_awgn_clean = vaeq_gen_awgn's first stage alone (sps == 2 only): the noise-free channel output sig[R][Ls] (complex64), the power sums
 * power_ws[R][ceil(Ls / 2048)] of its tiles and the TX reference data_f16[R][2][N].
 * vaeq_awgn_validate_gen = vaeq_awgn_validate on x = sig + noise, the noise added where a tile is staged: the Philox words, sigma_n (from
 * power_ws and snr_db, or sigma_fixed) and the arithmetic of vaeq_gen_awgn -- ser / shift / y_ws are bit for bit what vaeq_gen_awgn followed by
 * vaeq_awgn_validate return for the same (seed, frame) (sps == 2, M in {9, 17, 25}; VAEQ_ERR_SHAPE otherwise); sigma_out[R] nullable. */
int vaeq_gen_awgn_clean(int32_t R, int32_t N, int32_t N_conv, int32_t sps, int32_t n_lev, int32_t Lg, int32_t Ls, int32_t ref_offset,
                        const float *amp, const float *cdf, const float *g_complex, uint64_t seed, uint32_t frame, float *sig,
                        float *power_ws, void *data_f16, void *stream);
int vaeq_awgn_validate_gen(int32_t R, int64_t N, int32_t sps, int32_t M, int32_t n_lev, int32_t n_shift, const float *sig, int32_t Ls,
                           const float *power_ws, const float *snr_db, const float *sigma_fixed, uint64_t seed, uint32_t frame,
                           const float *W, const float *amp, const float *amp_mean, const float *var, const void *data_f16, float *y_ws,
                           float *ser, int32_t *shift, float *sigma_out, void *stream);

/* ------------------------------------------------------------------------
 * the constant-modulus baselines of the DP scripts and their carrier phase estimation.
 * vaeq_cma: CMA (shared_funcs.py:341-383, mode 0) / CMAbatch (:385-433, mode 1 with symb_step = batchlen) / CMAflex (:435-488,
 * mode 1) on one frame per run: rx[R][2][2][N] -> out[R][2][2][N/sps], e[R][N/sps][2] (nullable); taps h[R][2][2][2][M] and the
 * per-run step size lr[R] as in the reference (h is updated in place; R_mod is the modulus constant `R` of the reference).
 * vaeq_cpe: Viterbi-Viterbi carrier phase estimation (:139-186), y[R][2][2][N] -> y_out[R][2][2][N], M_ma = 501 in the reference. */
int vaeq_cma(int32_t R, int64_t N, int32_t sps, int32_t M, int32_t mode, int32_t batchlen, int32_t symb_step, const float *rx, float R_mod,
             float *h, const float *lr, float *out, float *e, void *stream);
int vaeq_cpe(int32_t R, int64_t N, int32_t M_ma, const float *y, float *y_out, void *stream);

/* ------------------------------------------------------------------------
 * The constant-modulus baseline of the AWGN scripts (AWGN_channel/func_CMA_MQAM_shaping.py, Eval_run_shaping_cma.py): ONE complex FIR,
 * no input power scaling, a CPE without unwrapping, its own shift search -- not vaeq_cma / vaeq_cpe with one polarisation removed.
 * vaeq_awgn_cma: CMA(Rx, R, h, lr, sps, eval) (:142-168) on one frame per run: rx[R][2][N] (re, im), taps h[R][2][M] (re, im; updated in place
 * when update != 0, untouched otherwise = eval False), lr[R] -> loss[R] = mean |e|, out[R][2][N/sps] and e[R][N/sps] (both nullable) at the
 * reference's wrapped indices.  M odd <= 63, 1 <= sps <= 8, N a multiple of sps, N / sps >= M.
 * vaeq_awgn_cma_validate: one evaluated epoch (:225-232) -- CMA(..., False) with the taps h, CPE (:170-198), find_shift_symb(., ., n_shift)
 * (:127-140) and SER_CMA (:63-94) -- in one launch: data_f16[R][2][N/sps] (TX, fp16), amp[n_lev] -> ser[R], shift[R] (nullable),
 * cpe_out[R][2][N/sps] (nullable: the CPE output).  n_lev in {2, 4, 8}, n_shift odd <= 23, N / sps >= 1000 + n_shift (the shift search
 * reads the first 1000 symbols).  ws: vaeq_awgn_cma_validate_ws_bytes(R, N, sps) bytes of device workspace -- 0 (ws may be NULL) while a
 * run's equalised track fits in LDS (N / sps <= 17408), R * 2 * (N / sps) * 8 otherwise. */
int vaeq_awgn_cma(int32_t R, int64_t N, int32_t sps, int32_t M, int32_t update, const float *rx, float R_mod, float *h, const float *lr,
                  float *loss, float *out, float *e, void *stream);
int vaeq_awgn_cma_validate(int32_t R, int64_t N, int32_t sps, int32_t M, int32_t n_lev, int32_t n_shift, const float *rx, const float *h,
                           const float *amp, const void *data_f16, float *ws, float *ser, int32_t *shift, float *cpe_out, void *stream);
int64_t vaeq_awgn_cma_validate_ws_bytes(int32_t R, int64_t N, int32_t sps);

/* ------------------------------------------------------------------------
 * The known-channel ("genie") baselines of AWGN_channel/DFE_MQAM_shaping.py at sps = 1 (the only setting of the script; VAEQ_ERR_SHAPE
 * otherwise).  rx[R][2][N] (re, im), data_f16[R][2][N] (TX, fp16), amp[n_lev] (n_lev in {2, 4, 8}), complex taps [R][2][K] (re, im), one
 * set per frame.  N >= 1000 + n_shift + 2 n_cut + 22 (the shift search reads the first 1000 symbols; n_shift / 2 <= n_cut + 11).
 * vaeq_awgn_lmmse_eval: compl_conv(rx, lmmse_taps) (:236-241, K even <= 64 -> N + 1 outputs), nearest_neighbor(out[1::1]) (:275),
 * find_shift_symb(out, data, n_shift) (:280) and SER_func(out[:, n_cut+11+shift : -11-n_cut], data[:, n_cut+11 : -11-shift-n_cut]) (:281,
 * the rescale over the one-sample-longer output slice) -> ser[R], shift[R] (nullable), dec[R][N] int8 (nullable: the per-symbol decisions
 * iI * n_lev + iQ), out[R][N+1] complex64 (nullable; the track lives in ws, vaeq_awgn_lmmse_eval_ws_bytes(R, N, K) bytes, when NULL).
 * vaeq_awgn_dfe: compl_conv(rx, ff_taps) (K1 <= 64 taps, :285), dfe(ff, ff_taps, fb_taps, init_dec) (:200-222, K2 = len(fb) in 1..10,
 * init_dec[R][N] = the LMMSE decisions) -> dec[R][N] int8, then find_shift_symb(., ., n_shift) and SER_func on the hard decisions (:290-293)
 * -> ser[R] (nullable: no evaluation, and no rule on N, n_shift, n_cut), shift[R] (nullable).  The recursion runs as speculate-and-repair over C chunks of ceil((N - K2) / C)
 * symbols (1 <= C <= 8192, each chunk at least K2 long) with W symbols of warm-up; the decisions are bit-identical for every C and W (C = 1
 * is the plain serial recursion).  repairs[R] (nullable): symbols the repair pass re-ran; ff_out[R][N] complex64 (nullable): the
 * feed-forward output.  ws: vaeq_awgn_dfe_ws_bytes(R, N, C) bytes. */
int vaeq_awgn_lmmse_eval(int32_t R, int64_t N, int32_t sps, int32_t n_lev, int32_t K, int32_t n_shift, int32_t n_cut, const float *rx,
                         const float *taps, const float *amp, const void *data_f16, float *ws, float *ser, int32_t *shift, int8_t *dec,
                         float *out, void *stream);
int64_t vaeq_awgn_lmmse_eval_ws_bytes(int32_t R, int64_t N, int32_t K);
int vaeq_awgn_dfe(int32_t R, int64_t N, int32_t sps, int32_t n_lev, int32_t K1, int32_t K2, int32_t C, int32_t W, int32_t n_shift,
                  int32_t n_cut, const float *rx, const float *ff_taps, const float *fb_taps, const float *amp, const int8_t *init_dec,
                  const void *data_f16, void *ws, int8_t *dec, float *ser, int32_t *shift, int32_t *repairs, float *ff_out, void *stream);
int64_t vaeq_awgn_dfe_ws_bytes(int32_t R, int64_t N, int32_t C);

/* Information-rate figures of the AWGN baselines, per run, on a complex soft sequence ("track") z in memory, over exactly the symbols the SER of
 * its validator keeps.  All three baselines end in one shape: z of Nz samples against TX data of Nd symbols through z[:, e+sh : -e] and
 * data[:, e : -e-sh], sh = shift[r], e = edge: 11 for the constant-modulus script (func_CMA_MQAM_shaping.py:231-232, z = cpe_out of
 * vaeq_awgn_cma_validate, planar [R][2][Nz]: interleaved = 0), N_cut + 11 = 31 for the LMMSE and the DFE (DFE_MQAM_shaping.py:281, :293; z = out of
 * vaeq_awgn_lmmse_eval, Nz = Nd + 1, or the z of vaeq_awgn_dfe_soft, Nz = Nd; [R][Nz][2]: interleaved = 1).
 * Window: L = Nd - 2 e - sh symbols are kept, the slice of z holds Lz = Nz - 2 e - sh samples; kept symbol j < L pairs z[e + sh + j] with TX
 * symbol e + j.  It is empty when e + sh <= 0 or L <= 0 (the reference's -0 slice), computed in 64 bits: no int32 shift takes an index out of a
 * row, and shifts are not clamped (find_shift_symb(., ., 24) returns -12 .. +11).
 * Normalisation (SER_CMA :73 = SER_func :117): scale = (sum_{j<L} |tx_j| / L) / (sum_{m<Lz} |z[e+sh+m]| / Lz), |.| the complex radius, over ALL Lz
 * samples of the slice; zhat = z scale.  A slice whose sum of |z| is zero has no normalisation: the empty-window result.
 * Demapper: the AWGN reference's own (func_VAELE_MQAM_shaping.py:229), per axis v_i = -(zhat_c - a_i)^2 / var[r], posteriors = log-softmax of v:
 * no 1/2 and no prior term, so the first maximum of the posterior is the nearest level.  var[R] is the caller's; the host layers pass
 * 10^(-SNR/10) (:272), what the VAE-LE of the same sweep point uses.
 * Gray labels, H, TX level, the four hypotheses (the relabelings of SER_CMA / SER_func: 0, pi, pi/2, 3 pi/2, in that order), tie-break, AIR, GMI,
 * BER, the K == 0 rule and the outputs are vaeq_awgn_info's y-mode: data_f16[R][2][Nd] IEEE half, amp[n_lev], P[R][n_lev] the runs' per-axis pmf
 * -> info[R][3] = AIR, GMI, BER; counts[R][4] = kept, sym_err, bit_err, hyp (NGMI is the host's).  The kernel decides with its own radius sums,
 * so sym_err / kept is the validator's SER except where a sample lies within float32 rounding of a decision threshold.  (The DFE's validator
 * scores the HARD decisions, whose mean radius SER_func normalises; the figures normalise the soft sequence, whose mean radius the noise raises a
 * little.  A slicer input within that difference of a threshold -- a fraction of a per cent of a level spacing -- is decided the other way: at low
 * SNR sym_err can differ from SER kept by a symbol or two.)
 * One launch, one 256-thread workgroup per run, a pre-pass for the two radius sums and one pass over the window; sums run in a fixed order without
 * atomics: two calls give identical bits, R runs in one call the bits of R single calls.
 * R == 0 is VAEQ_OK (its pointers may be NULL); any NULL pointer is VAEQ_ERR_NULL, before any shape rule; R < 0, Nd < 1, Nz not in {Nd, Nd + 1},
 * Nz > 0x3fffffff, edge < 0, interleaved not in {0, 1} or n_lev not in {2, 4, 8} is VAEQ_ERR_SHAPE. */
int vaeq_awgn_track_info(int32_t R, int64_t Nz, int64_t Nd, int32_t n_lev, int32_t edge, int32_t interleaved, const float *z,
                         const void *data_f16, const float *amp, const float *P, const float *var, const int32_t *shift, float *info,
                         int32_t *counts, void *stream);

/* The per-bit a-posteriori LLRs of an AWGN baseline's soft sequence, under the definition of vaeq_dp_epilogue_llr with the four rotation hypotheses
 * of vaeq_awgn_track_info (hyp[R] = its counts[..][3], used as hyp & 3; no IQ flip) and that call's window, layouts, normalisation and demapper:
 * z planar [R][2][Nz] (interleaved = 0) or [R][Nz][2] (interleaved = 1), data_f16[R][2][Nd] (needed for the normalisation only), amp[n_lev], var[R],
 * shift[R] unclamped, the window in 64 bits.  scale = (sum_{j<L} |tx_j| / L) / (sum_{m<Lz} |z[e+sh+m]| / Lz) over ALL Lz samples of the slice, summed
 * in that kernel's order so that the LLRs are those of the posteriors whose GMI it reports; v_i = -(zhat_c - a_i)^2 / var, each bit-wise set a
 * log-sum-exp around its own maximum.
 * llr[R][2 b][Nd] float32, nats, positive = bit 0: plane a b + k holds bit k of TX axis a, indexed by the TX symbol index; TX index e + j, j < L,
 * holds the LLRs of sample e + sh + j.  Everything else is an erasure, written as +0.0, and an empty window or a slice whose sum of |z| is zero
 * writes the whole row as zeros (the buffer may be uninitialised: every entry is written).
 * One 256-thread workgroup per run, a pre-pass and one elementwise pass; no atomics: two calls give identical bits.
 * R == 0 is VAEQ_OK (its pointers may be NULL); any NULL pointer is VAEQ_ERR_NULL, before any shape rule; R < 0, Nd < 1, Nz not in {Nd, Nd + 1},
 * Nz > 0x3fffffff, edge < 0, interleaved not in {0, 1} or n_lev not in {2, 4, 8} is VAEQ_ERR_SHAPE. */
int vaeq_awgn_track_llr(int32_t R, int64_t Nz, int64_t Nd, int32_t n_lev, int32_t edge, int32_t interleaved, const float *z,
                        const void *data_f16, const float *amp, const float *var, const int32_t *shift, const int32_t *hyp, float *llr,
                        void *stream);

/* The DFE's soft sequence.  The reference's dfe() leaves only hard decisions; its soft value is the slicer input (DFE_MQAM_shaping.py:215-221),
 * rebuilt here from what vaeq_awgn_dfe returns: ff[R][N] complex64 (ff_out), fb[R][2][K2] (re, im; the feedback taps), dec[R][N] int8, amp[n_lev]
 *   z[p] = ff[p] + sum_{j < K2} fb[j] c(dec[p - 1 - j]) for p >= K2,   c(i) = amp[i / n_lev] + j amp[i % n_lev]
 * -- plain complex products without conjugation, added to the feed-forward sample with j ascending -- and z[p] = c(dec[p]) for p < K2, the state the
 * reference holds where no slicer input exists.  z[R][N] complex64.  One thread per sample.
 * R == 0 is VAEQ_OK (its pointers may be NULL); any NULL pointer is VAEQ_ERR_NULL, before any shape rule; R < 0, N < 1, N > 0x3fffffff, n_lev not
 * in {2, 4, 8} or K2 outside 1 .. 10 (vaeq_awgn_dfe's range) is VAEQ_ERR_SHAPE. */
int vaeq_awgn_dfe_soft(int32_t R, int64_t N, int32_t n_lev, int32_t K2, const float *ff, const float *fb, const int8_t *dec, const float *amp,
                       float *z, void *stream);

/* Post-FEC figures on the device: a batched decoder of quasi-cyclic LDPC codes over the per-bit LLRs of the calls above (no reference counterpart:
 * the reference stops at the SER).  The code: shifts_host[mb][nb] int32 in HOST memory, -1 = a zero block, 0 <= s < Z = a Z x Z circulant that
 * connects check l Z + i to variable c Z + (i + s) mod Z; n = nb Z bits, m = mb Z checks.  The table is validated on every call and travels to
 * the kernel by value in its arguments (no copy from pageable memory, nothing to keep alive).
 * llr[R][w][N] float32 (positive = bit 0) and bits[R][w][N] int8 (the TX bits): the DP tensors [R][2][2b][N] with w = 4 b, the AWGN tensors with
 * w = 2 b.  Bit j of codeword c of a run is global bit g = c n + j: symbol t0 + g / w, plane g % w -- symbol-major, so a codeword mixes all bit
 * levels (and both polarisations) as BICM needs; n % w may be non-zero.  C codewords per run, t0 w + C n <= N w.
 * No encoder: the TX bits are not a codeword, so the decoder works towards their syndrome sigma = H bits mod 2 (coset decoding).
 * Layered normalized min-sum in float32, every multiply, add and subtract rounded on its own (nothing contracts to a fused multiply-add), in
 * this order, so that a float32 model reproduces every bit:
 *   start      L[v] = llr of bit v; sigma_i = parity of the TX bits on check i; every check's (m1, m2, idx, signs) = (0, 0, 0, 0).
 *   negative   means x < 0: +-0 is bit 0, for the hard decisions x_v = (L[v] < 0) and for message signs alike.
 *   test       H x = sigma, before the first iteration and after every full one; decoding stops at success or after max_iter iterations.
 *   iteration  layers l = 0 .. mb - 1 in order; in layer l check i takes its edges e = 0, 1, .. in ascending block column, v_e its variable:
 *              r_e = +-(alpha m2 if e == idx else alpha m1) from the check's stored state, negative iff bit e of signs;  t_e = L[v_e] - r_e;
 *              m1, m2 = the smallest and second smallest |t_e|, idx = the first edge that attains m1;  s_e = (t_e < 0), S = xor_e s_e xor sigma_i;
 *              r'_e = +-(alpha m2 if e == idx else alpha m1) of the NEW state, negative iff S xor s_e;  L[v_e] = t_e + r'_e.
 *              (The checks of a layer own disjoint variables: they run in parallel with the result of any serial order.)
 * out[R][C][5] int32 = iters (full iterations executed: 0 for a codeword that passes the first test), ok (the test passed at exit), post_err
 * (decisions of the final L against the TX bits, over the n bits), pre_err (the same of the input), erased (inputs equal to +-0).
 * post[R][C][n] float32 (nullable): the final L in codeword order.
 * The LLRs must not be NaN here: what a NaN does to the minimum search is not fixed (vaeq_ldpc_decode_q maps a NaN to +0).
 * One workgroup per codeword, one thread per check of the layer in flight, the whole state in LDS: vaeq_ldpc_lds_bytes(mb, nb, Z) bytes (L,
 * the TX bits as bytes, 16 bytes per check), VAEQ_ERR_SHAPE from that call outside the ranges of mb, nb and Z below.  Integer counts and a
 * fixed operation order: two calls give identical bits.
 * R == 0 is VAEQ_OK (its pointers may be NULL); a NULL shifts_host, llr, bits or out is VAEQ_ERR_NULL, before any shape rule; VAEQ_ERR_SHAPE, all
 * before any HIP call: R < 0, C < 1, R C > 0x7fffffff, N < 1, N > 0x3fffffff, w outside 1 .. 64, t0 < 0, t0 w + C n > N w, max_iter outside
 * 1 .. 100, mb outside 1 .. 8, nb outside 2 .. 64, Z outside 2 .. 512, a state above 64 KiB, a shift < -1 or >= Z, a block row with fewer than 2 or
 * more than 32 non-zero blocks. */
int vaeq_ldpc_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t mb, int32_t nb, int32_t Z, const int32_t *shifts_host,
                     const float *llr, const int8_t *bits, float alpha, int32_t max_iter, int32_t *out, float *post, void *stream);
int64_t vaeq_ldpc_lds_bytes(int32_t mb, int32_t nb, int32_t Z);

/* vaeq_ldpc_decode behind a symbol interleaver over groups of `depth` codewords, so that a burst of bad symbols (the DFE's error propagation,
 * a tracking transient at the head of a frame) is shared among the codewords of a group and does not fall on one of them.
 * S = ceil(n / w) symbols per codeword: codewords are symbol-aligned here, not bit-packed.  Group k holds the codewords k depth ..
 * min((k + 1) depth, C) - 1: D_k of them, depth except in a ragged last group.  Its base is symbol t0 + k depth S, and bit j of the codeword
 * with local index d of group k is symbol base + (j / w) D_k + d, plane j % w.  When n % w != 0, the planes >= n - (S - 1) w of a codeword's
 * last symbol belong to no codeword: they are never loaded into L and never counted in pre_err or erased.  depth == 1: symbol-aligned contiguous
 * codewords; depth == C: symbol u of codeword c is symbol t0 + u C + c, every codeword spread over the whole used part of the frame.
 * Everything else -- the code, the tensors, the algorithm and its float32 operation order, out[R][C][5] and post[R][C][n] in codeword order,
 * the state in LDS -- is vaeq_ldpc_decode's.  The refusals are vaeq_ldpc_decode's too, in its order and all before any HIP call, but for:
 * depth < 1 or depth > C is VAEQ_ERR_SHAPE, and the fit rule is t0 + C S > N is VAEQ_ERR_SHAPE. */
int vaeq_ldpc_decode_il(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t mb, int32_t nb, int32_t Z,
                        const int32_t *shifts_host, const float *llr, const int8_t *bits, float alpha, int32_t max_iter, int32_t *out, float *post,
                        void *stream);

/* The fixed-point decoder: vaeq_ldpc_decode's layered min-sum with q-bit channel LLRs, q-bit check messages and saturating a-posteriori values,
 * as a hardware decoder holds them.  Float32 normalized min-sum is positively homogeneous: a common factor on every LLR changes no decision and
 * no counter, so vaeq_ldpc_decode cannot show whether an equalizer's noise-variance estimate (the scale of its LLRs) is any good.  Here the
 * scale decides what is clipped and what rounds to an erasure.
 * The code table, the tensors llr[R][w][N] / bits[R][w][N], coset decoding towards the syndrome of the TX bits, the layer order, the edge order
 * (ascending block column), the test before the first and after every full iteration, and out[R][C][5] are vaeq_ldpc_decode's.  depth == 0 is
 * vaeq_ldpc_decode's bit-packed contiguous mapping with its fit rule, depth >= 1 vaeq_ldpc_decode_il's symbol interleaver with its fit rule.
 * Everything behind the quantiser is integer arithmetic, fixed here so that an integer model reproduces every bit:
 *   constants  Cmax = Mmax = 2^(qbits-1) - 1, Lmax = 2^(abits-1) - 1.
 *   quantiser  (the only float operations, each rounded on its own)  x = llr * scale in float32; a NaN x becomes +0; x = min(max(x, -Cmax), Cmax);
 *              Q = rint(x), ties to even, as an integer.
 *   counters   pre_err counts (llr < 0) != bit on the RAW float input (vaeq_ldpc_decode's pre_err of the same tensors; a NaN is bit 0);
 *              erased counts Q == 0: what the quantiser erased, not only exact zeros.
 *   start      L[v] = Q[v]; every check's (m1, m2, idx, signs) = (0, 0, 0, 0).  Negative means < 0: integer 0 is bit 0.
 *   f          f(m) = max(((num m + 4) >> 3) - beta, 0): num = 6, beta = 0 is alpha = 0.75 rounded half up; num = 8, beta = 1 plain offset min-sum.
 *   layer      for check i with edges e:  r_e = +-f(m2 if e == idx else m1) of the stored state, negative iff bit e of signs;
 *              t_e = L[v_e] - r_e, exact (|t_e| <= Lmax + Mmax fits 16 bits because abits <= 15);  a_e = min(|t_e|, Mmax);
 *              m1, m2 = the smallest and second smallest a_e, idx = the FIRST edge that attains m1 after the clamp (ties are the common case);
 *              s_e = (t_e < 0), S = xor_e s_e xor sigma_i;  r'_e = +-f(m2 if e == idx else m1) of the NEW state, negative iff S xor s_e;
 *              L[v_e] = min(max(t_e + r'_e, -Lmax), Lmax).
 * post[R][C][n] int16 (nullable): the final L in codeword order; post_err counts L < 0 against the TX bits.
 * One workgroup per codeword as in vaeq_ldpc_decode, the state in LDS: vaeq_ldpc_q_lds_bytes(mb, nb, Z) = 2 n (L as int16, padded to a word)
 * + n (the TX bits as bytes, padded to a word) + 8 m (one dword m1 | m2 << 8 | idx << 16 | sigma << 24 and one dword of signs per check), at most
 * 64 KiB; VAEQ_ERR_SHAPE from that call outside the ranges of mb, nb and Z.  Integers and a fixed order: two calls give identical bits.
 * Refusals, all before any HIP call and in vaeq_ldpc_decode's order: R == 0 is VAEQ_OK (its pointers may be NULL); a NULL shifts_host, llr, bits
 * or out is VAEQ_ERR_NULL, before any shape rule; then VAEQ_ERR_SHAPE for vaeq_ldpc_decode's shape rules with this state size and the fit rule of
 * the depth, and for qbits outside 2 .. 8, abits outside qbits .. 15, a scale that is not finite or <= 0, num outside 1 .. 8, beta outside
 * 0 .. 127, depth < 0 or depth > C, and last the table's rules. */
int vaeq_ldpc_decode_q(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t mb, int32_t nb, int32_t Z,
                       const int32_t *shifts_host, const float *llr, const int8_t *bits, int32_t qbits, int32_t abits, float scale, int32_t num,
                       int32_t beta, int32_t max_iter, int32_t *out, int16_t *post, void *stream);
int64_t vaeq_ldpc_q_lds_bytes(int32_t mb, int32_t nb, int32_t Z);

/* Spatially coupled LDPC codes with a sliding-window decoder: a terminated chain of Lc positions, far longer than what vaeq_ldpc_decode can hold
 * in LDS, decoded by a window of W row-block positions that slides along it (no reference counterpart).
 * The code: components_host[ms + 1][mb][nb] int32 in HOST memory, -1 = a zero block, 0 <= s < Z = vaeq_ldpc_decode's Z x Z circulant (check i to
 * variable (i + s) mod Z of its block).  The coupled matrix has block rows (t, l), t = 0 .. Lc + ms - 1, l = 0 .. mb - 1, row block index t mb + l,
 * and block columns (i, c), i = 0 .. Lc - 1, c = 0 .. nb - 1, column block index i nb + c; block ((t, l), (i, c)) is components[t - i][l][c] when
 * 0 <= t - i <= ms and zero otherwise.  n_chain = Lc nb Z bits, (Lc + ms) mb Z checks, design rate 1 - (Lc + ms) mb / (Lc nb); the chain is
 * terminated, its first and last ms row blocks are lighter.
 * The tensors llr[R][w][N], bits[R][w][N] and the bit map are vaeq_ldpc_decode's with n = n_chain: C chains per run, bit j of chain c is global
 * bit g = c n_chain + j at symbol t0 + g / w, plane g % w, and t0 w + C n_chain <= N w.  Column block i of chain c is thus codeword c Lc + i of
 * nb Z bits of that map.  No encoder: coset decoding towards the syndrome of the TX bits.
 *   start      as in vaeq_ldpc_decode: L[v] = llr of bit v, sigma = the parity of the TX bits on each check, every check's (m1, m2, idx, signs)
 *              zero; pre_err and erased are counted on the input over the n_chain bits.
 *   positions  p = 0 .. P - 1, P = max(1, Lc + ms - W + 1).  The active rows at p are t in [p, min(p + W, Lc + ms)), every l.
 *   test       H x = sigma on the hard decisions L < 0, restricted to the rows t in [p, min(p + T, Lc + ms)) for p < P - 1 and to all active
 *              rows at the last position; before the first iteration of a position and after every full one.  The position ends at success
 *              or after `iters` iterations.
 *   iteration  the active layers in ascending (t, l), each exactly vaeq_ldpc_decode's layer update with the same float32 operations, each
 *              rounded on its own; the edges of a check in ascending coupled block column: i ascending (t - i descending), then c ascending;
 *              idx = the first edge that attains m1.  Edges whose i falls outside [0, Lc) do not exist.
 *   between    nothing is reset.  Rows that stay keep their state, row p is never visited again, row p + W starts from zeros when it enters.
 *              Column blocks p - ms .. p - 1 stay in the window and are updated like any other (they are not frozen).  Column block i is
 *              final once position min(i + ms, P - 1) has ended.
 * out[R][C][6] int32 = iters (the sum over the positions), ok (1 iff the last test of every position passed), post_err (the final decisions
 * against the TX bits over n_chain), pre_err, erased, iters_max (the most iterations at any one position).  Nullable: post[R][C][n_chain]
 * float32, the final L; pos_err[R][C][Lc] int32, the errors of each column block in its final state (the decoding wave, and how errors
 * propagate along the chain); pos_iters[R][C][P] int32, the iterations of each position.
 * When W >= Lc + ms there is one position and its test covers every row: the call equals vaeq_ldpc_decode on the coupled
 * shifts[(Lc + ms) mb][Lc nb] with max_iter = iters, in the five shared counters and in every bit of post.
 * One workgroup per chain, one thread per check of the layer in flight.  The window is a ring in LDS, vaeq_ldpc_sc_lds_bytes(ms, mb, nb, Z, W):
 * W + ms column blocks (L as float32, the TX bits as bytes padded to a word) and 16 bytes per check of W row blocks; VAEQ_ERR_SHAPE from that
 * call outside the ranges of ms, mb, nb, Z and W below.  The LLRs must not be NaN.  Integer counts and a fixed order: two calls give identical bits.
 * Refusals, all before any HIP call and in vaeq_ldpc_decode's order: R == 0 is VAEQ_OK (its pointers may be NULL); a NULL components_host, llr,
 * bits or out is VAEQ_ERR_NULL, before any shape rule; then VAEQ_ERR_SHAPE for R < 0, C < 1, N < 1, N > 0x3fffffff, w outside 1 .. 64, t0 < 0,
 * t0 > N, iters outside 1 .. 100, ms outside 1 .. 7, mb outside 1 .. 4, nb outside 2 .. 32, Z outside 2 .. 512, W outside ms + 1 .. 32, Lc outside
 * 1 .. 65535, T outside 1 .. W; for a state above 64 KiB, t0 w + C n_chain > N w, R C > 0x7fffffff and C Lc > 0x7fffffff (a column block's
 * codeword index); last for the table: a shift < -1 or >= Z, an l with more than 32 non-zero blocks over its ms + 1 components, a block row
 * (t, l) of the coupled matrix with fewer than 2 non-zero blocks, the truncated rows at both ends counted with the blocks they really have. */
int vaeq_ldpc_sc_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t ms, int32_t mb, int32_t nb, int32_t Z, int32_t Lc,
                        const int32_t *components_host, const float *llr, const int8_t *bits, int32_t W, int32_t T, float alpha, int32_t iters,
                        int32_t *out, float *post, int32_t *pos_err, int32_t *pos_iters, void *stream);
int64_t vaeq_ldpc_sc_lds_bytes(int32_t ms, int32_t mb, int32_t nb, int32_t Z, int32_t W);

/* The fixed-point window decoder: vaeq_ldpc_sc_decode's sliding window with vaeq_ldpc_decode_q's integer layer rule, as a hardware window decoder
 * holds its 4 to 6-bit LLRs and messages.  Like vaeq_ldpc_decode_q and unlike vaeq_ldpc_sc_decode it sees the scale of the LLRs.  Both comments
 * above hold word for word where they are named here; nothing of them is restated.
 * From vaeq_ldpc_sc_decode, unchanged: the code components_host[ms + 1][mb][nb], the coupled matrix, the tensors and the bit map with n = n_chain;
 * coset decoding without an encoder; the positions p = 0 .. P - 1, the active rows, the test rows T and when the test runs (on L < 0); the layer
 * order (ascending (t, l)) and the edge order (ascending coupled block column); "between": nothing is reset, a row starts from zeros when it
 * enters, and a column block is final once position min(i + ms, P - 1) has ended; out[R][C][6], pos_err[R][C][Lc] and pos_iters[R][C][P].
 * From vaeq_ldpc_decode_q, unchanged: the constants Cmax = Mmax and Lmax; the quantiser (float32 multiply, a NaN becomes +0, clamp, rint with ties
 * to even), applied to every bit of the chain; pre_err counted on the raw input and erased counting Q == 0, both over the n_chain bits; f; the
 * layer update in integers -- t_e exact, the clamp to Mmax before the minimum search, idx the first edge that attains m1 after the clamp,
 * L = min(max(t_e + r'_e, -Lmax), Lmax); negative means < 0.
 * Edge numbering: an edge's number e is its number in the full row (i ascending, then c ascending, over all ms + 1 components), wherever the row
 * lies in the chain.  Edges whose i falls outside [0, Lc) do not exist: they contribute no magnitude to m1 and m2, no sign to S, can not be the
 * specified idx, and nothing is written for them.
 * post[R][C][n_chain] int16 (nullable): the final L; post_err and pos_err count L < 0 against the TX bits.
 * When W >= Lc + ms there is one position and its test covers every row: the call equals vaeq_ldpc_decode_q with depth = 0 on the coupled
 * shifts[(Lc + ms) mb][Lc nb] with max_iter = iters and the same qbits, abits, scale, num and beta, in the five shared counters and in every bit
 * of post.
 * One workgroup per chain, one thread per check of the layer in flight.  The window is a ring in LDS, vaeq_ldpc_sc_q_lds_bytes(ms, mb, nb, Z, W) =
 * 2 (W + ms) nb Z (L as int16, padded to a word) + (W + ms) nb Z (the TX bits as bytes, padded to a word) + 8 W mb Z (one dword
 * m1 | m2 << 8 | idx << 16 | sigma << 24 and one dword of signs per check of W row blocks), at most 64 KiB; VAEQ_ERR_SHAPE from that call outside
 * the ranges of ms, mb, nb, Z and W, which are vaeq_ldpc_sc_decode's, as those of Lc, T and iters are.  Integers and a fixed order: two calls give
 * identical bits.
 * Refusals, all before any HIP call and in vaeq_ldpc_sc_decode's order: R == 0 is VAEQ_OK (its pointers may be NULL); a NULL components_host, llr,
 * bits or out is VAEQ_ERR_NULL, before any shape rule; then VAEQ_ERR_SHAPE for vaeq_ldpc_sc_decode's shape rules with this state size; then for
 * qbits outside 2 .. 8, abits outside qbits .. 15, a scale that is not finite or <= 0, num outside 1 .. 8, beta outside 0 .. 127; and last the
 * table's rules. */
int vaeq_ldpc_sc_decode_q(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t ms, int32_t mb, int32_t nb, int32_t Z, int32_t Lc,
                          const int32_t *components_host, const float *llr, const int8_t *bits, int32_t W, int32_t T,
                          int32_t qbits, int32_t abits, float scale, int32_t num, int32_t beta, int32_t iters,
                          int32_t *out, int16_t *post, int32_t *pos_err, int32_t *pos_iters, void *stream);
int64_t vaeq_ldpc_sc_q_lds_bytes(int32_t ms, int32_t mb, int32_t nb, int32_t Z, int32_t W);

/* The outer code behind the LDPC decoders: a bounded-distance hard-decision decoder of a shortened binary BCH code over the payload bits of
 * `post`, so that the figure an optical-FEC comparison is judged by -- errors after the outer code -- is counted on the device.  As with the inner
 * code there is no encoder: the result depends on the error pattern alone.
 * The code: narrow-sense primitive binary BCH over GF(2^m), m in 4 .. 13, designed correction t in 1 .. 16, shortened to n_o bits.  alpha is the
 * root of the primitive polynomial (bit masks, m = 4 .. 13) 0x13, 0x25, 0x43, 0x89, 0x11D, 0x211, 0x409, 0x805, 0x1053, 0x201B.  Position p of a
 * codeword belongs to alpha^p; shortening keeps the positions 0 .. n_o - 1.  parity(m, t) = the size of the union of the cyclotomic cosets of
 * 1 .. 2t modulo 2^m - 1, and parity < n_o <= 2^m - 1.
 * The payload: the first K bits of every LDPC codeword of n bits, 1 <= K <= n.  A run's payload stream has C K bits, stream bit u = c K + i is bit
 * i of LDPC codeword c.  C_o outer codewords per run, C_o n_o <= C K; stream bits past C_o n_o belong to no outer codeword.  spread == 0:
 * position p of outer codeword a is stream bit a n_o + p.  spread == 1: stream bit p C_o + a, a bit interleaver over all outer codewords of the
 * run, which turns one failed LDPC codeword into a few errors in each outer codeword.
 * The received bit is post[r][c][i] < 0 (a float NaN and +-0 are bit 0, as in the decoders); post[R][C][n] is float32 (post_i16 == 0) or int16
 * (post_i16 == 1), the `post` output of the three LDPC calls.  The transmitted bit is bits[r][plane][symbol] of the demappers' [R][w][N] tensor
 * under the LDPC decoder's own map of codeword c, bit i: depth == 0 vaeq_ldpc_decode's bit-packed map, depth >= 1 vaeq_ldpc_decode_il's;
 * t0, w, N, n and C as in those calls.  e = received xor transmitted is the error pattern of an outer codeword.
 * The rule, stated without an algorithm:  S_j = xor over the positions p with e_p = 1 of alpha^(j p), j = 1 .. 2t.
 *   status 0   every S_j is zero; nothing is flipped.
 *   status 1   there is a set of at most t positions, all below n_o, whose S_1 .. S_2t equal those of e.  That set is unique; it is flipped.
 *   status 2   otherwise; nothing is flipped.
 * (With an error locator Lambda of degree L: status 1 iff L <= t, Lambda has exactly L roots alpha^(-p), and all of them have p < n_o.)
 * out[R][C_o][4] int32 = status, pre_err (the weight of e), post_err (the weight after the flips), nflip.  loc[R][C_o][t] int16 (nullable): the
 * flipped positions ascending, padded with -1.  A miscorrection is status 1 with post_err > 0, an undetected error status 0 with pre_err > 0.
 * Workgroups of four waves, the exp / log tables of GF(2^m) in LDS (2^(m+2) bytes), one wave per outer codeword.  Integers only: two calls give
 * identical bits.
 * Refusals, all before any HIP call: R == 0 is VAEQ_OK (its pointers may be NULL); a NULL post, bits or out is VAEQ_ERR_NULL, before any shape
 * rule; then VAEQ_ERR_SHAPE for the tensor rules of the LDPC calls (R < 0, C < 1, R C > 0x7fffffff, N < 1, N > 0x3fffffff, w outside 1 .. 64,
 * t0 < 0, t0 > N), depth outside 0 .. C, n outside 2 .. 32768 and that depth's fit rule (t0 w + C n > N w, or t0 + C ceil(n / w) > N); then
 * VAEQ_ERR_SHAPE for K outside 1 .. n, m outside 4 .. 13, t outside 1 .. 16, n_o outside parity + 1 .. 2^m - 1, spread outside 0 .. 1, post_i16
 * outside 0 .. 1, C_o < 1 and R C_o > 0x7fffffff; last VAEQ_ERR_SHAPE for C_o n_o > C K. */
int vaeq_bch_outer(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t n, int32_t K, int32_t m, int32_t t, int32_t n_o,
                   int32_t C_o, int32_t spread, const void *post, int32_t post_i16, const int8_t *bits, int32_t *out, int16_t *loc, void *stream);

/* Hard-decision FEC: a staircase code over BCH components with a sliding-window iterative decoder, for the figure a coherent-optics comparison
 * quotes beside the soft-decision one -- whether the link is error-free behind a hard-decision FEC at a given pre-FEC BER (no reference
 * counterpart).  No encoder: every component code is linear and bounded-distance decoding depends on the error pattern alone, so the whole
 * iterative decoder, miscorrections included, acts on e = received xor transmitted exactly as it would on a transmitted codeword.
 * The component code: vaeq_bch_outer's narrow-sense primitive binary BCH code over GF(2^m) -- the same polynomials, position p belongs to
 * alpha^p -- with designed correction t, shortened to 2 s bits; parity(m, t) as there, and parity(m, t) < 2 s <= 2^m - 1.
 * The chain: L transmitted blocks B_1 .. B_L of s x s bits; B_0 is not transmitted, it is all zero and is never flipped.  n_chain = L s^2.  The
 * tensors llr[R][w][N] / bits[R][w][N] and the bit-packed map are vaeq_ldpc_decode's: C chains per run, bit (a, b) of block i of chain c is
 * global bit g = c n_chain + (i - 1) s^2 + a s + b at symbol t0 + g / w, plane g % w, and t0 w + C n_chain <= N w.  The received bit is
 * llr < 0: a NaN and +-0 are bit 0, as in the decoders.
 *   components pair i (1 .. L) has the components j = 0 .. s - 1, each the word [column j of B_(i-1) | row j of B_i]: position p < s is bit (p, j)
 *              of block i - 1, position s + p' is bit (j, p') of block i.
 *   rule       a component is decided by vaeq_bch_outer's rule with n_o = 2 s on its part of e: status 0, nothing flipped; status 1, the unique
 *              set of at most t positions with the component's syndromes is flipped; status 2, nothing flipped.  One addition: in pair 1 a set
 *              that contains a position below s is status 2 -- B_0 holds nothing to flip, and without this rule a miscorrection writes errors
 *              into a block that does not exist.
 *   positions  q = 0 .. P - 1, P = max(1, L - W + 1).  The active pairs at q are i = q + 1 .. min(q + W, L).
 *   iteration  the active pairs in ascending i.  In a pair step every component is decided on the state before the step, then all flips are
 *              applied (a pair's components own disjoint bits: this equals any sequential order).  A position ends after an iteration that
 *              flips nothing, which is counted, or after `iters` iterations.
 *   between    nothing is reset.  Block i is final once position min(i, P - 1) has ended.
 * out[R][C][8] int32, the first six in vaeq_ldpc_sc_decode's layout: iters (the sum over the positions), ok (1 iff at every position the last
 * executed iteration had every active component at status 0), post_err (errors after decoding, over n_chain), pre_err (errors before), erased
 * (inputs equal to +-0), iters_max (the most iterations at any one position), nflip (all flips), bad_flips (flips of a bit whose error bit was
 * 0 at that moment: what miscorrection costs).  Nullable: hard[R][C][n_chain] int8, the final decisions (the TX bit xor the final error bit);
 * pos_err[R][C][L] int32, the errors of blocks 1 .. L in their final state; pos_iters[R][C][P] int32.
 * The last block is protected by one component per bit, not by two like every other: it keeps more errors than the steady state of the chain,
 * and a short chain's post_err is mostly its tail.  pos_err is how a user reads the steady state: the blocks before the last.
 * One workgroup per chain, one lane per component of the pair in flight.  The state in LDS is vaeq_staircase_lds_bytes(m, s, W) = 4 2^m (the
 * exp and log tables of GF(2^m), uint16) + 8 (W + 1) s ceil(s / 32) (the error pattern of the window's W + 1 blocks as bitmaps, each block
 * row-major and transposed, a row in whole 32-bit words), at most 64 KiB; VAEQ_ERR_SHAPE from that call for m outside 4 .. 10, s outside
 * 2 .. 511, 2 s > 2^m - 1 or W outside 1 .. 32.  That figure and its bound are the state a caller sizes, the kernel's dynamic LDS; the kernel
 * keeps a few hundred bytes of counters in static LDS besides (416 as built: profiles/staircase/scan_isa.txt), so the largest accepted
 * shape holds 65 936 bytes per workgroup, of the 160 KiB of a gfx950 CU.  Integers and a fixed order: two calls give identical bits.
 * The counts are 32 bits wide while the envelope admits a chain of more than 2^31 bits (L s^2 reaches 1.7e10): post_err, pre_err, erased and
 * pos_err are exact for n_chain < 2^31, nflip and bad_flips while the flips stay below 2^31, and past that each is the count modulo 2^32.
 * Refusals, all before any HIP call and in vaeq_ldpc_sc_decode's order: R == 0 is VAEQ_OK (its pointers may be NULL); a NULL llr, bits or out is
 * VAEQ_ERR_NULL, before any shape rule; then VAEQ_ERR_SHAPE for the tensor rules of the LDPC calls (R < 0, C < 1, N < 1, N > 0x3fffffff, w
 * outside 1 .. 64, t0 < 0, t0 > N), iters outside 1 .. 100, m outside 4 .. 10, t outside 1 .. 8, s outside 2 .. 511, 2 s > 2^m - 1,
 * parity(m, t) >= 2 s, L outside 1 .. 65535, W outside 1 .. 32; then for a state above 64 KiB, t0 w + C n_chain > N w (decided
 * without forming C n_chain, which passes 2^63 inside the envelope) and R C > 0x7fffffff. */
int vaeq_staircase_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t m, int32_t t, int32_t s, int32_t L,
                          const float *llr, const int8_t *bits, int32_t W, int32_t iters,
                          int32_t *out, int8_t *hard, int32_t *pos_err, int32_t *pos_iters, void *stream);
int64_t vaeq_staircase_lds_bytes(int32_t m, int32_t s, int32_t W);

/* The inner code in front of the hard-decision FEC: a soft-in / hard-out Chase decoder of a short single-error-correcting code over the demappers'
 * LLRs, as a concatenated scheme such as 400ZR's places a Hamming-type word in front of its staircase code (no reference counterpart).  No encoder:
 * the code is linear and the rule symmetric, so it acts on e = received xor transmitted exactly as it would on a transmitted codeword.
 * The code: cols_host[n] int32 in HOST memory, column j of the parity-check matrix as an r-bit integer; n in 3 .. 256, r in 2 .. 10, the columns
 * distinct, non-zero and below 2^r -- any such matrix corrects one error.  A Hamming code is cols[j] = j + 1, the extended Hamming code with d = 4
 * is cols[j] = (j << 1) | 1, either one shortened to its first n columns.  The table is validated on every call and travels to the kernel by value.
 * The tensors llr[R][w][N] / bits[R][w][N] and the bit map are vaeq_ldpc_decode's with this n, C codewords per run: depth == 0 its bit-packed map
 * and fit rule, depth >= 1 vaeq_ldpc_decode_il's symbol interleaver with its fit rule and its unused planes.
 * The rule for one codeword, in integers and float32 so that a numpy model reproduces every bit:
 *   input      x_j = the LLR of bit j, a NaN mapped to +0;  y_j = (x_j < 0): +-0 is bit 0;  a_j = |x_j| in float32, +inf allowed;
 *              e_j = y_j xor bit_j;  s0 = xor over the j with e_j = 1 of cols[j].
 *   positions  the n positions ordered by (a_j, j) ascending; l_0 .. l_(p-1) are the first p, the least reliable; p in 0 .. min(6, n).
 *   patterns   T = 0 .. 2^p - 1:  F_T = { l_i : bit i of T };  s_T = s0 xor (xor over F_T of cols).  s_T == 0: the candidate of T flips F_T.
 *              s_T == cols[v] (v is unique): the candidate flips the symmetric difference of F_T and {v}.  Otherwise T has no candidate.
 *   metric     of a candidate: from +0.0f, add a of its flipped positions one float32 addition at a time -- the members of F_T in ascending i,
 *              without v where v cancelled a member, then v last where it was added.  (x + (+0.0f) = x bit for bit for every x >= +0, so an
 *              addition predicated to +0.0f is the same sum; the kernel adds that way.)
 *   winner     the candidate with the smallest (metric, T), the metric compared as a number (= as its bit pattern: it is never negative).
 *   status 0   the winner flips nothing; this is the case exactly when s0 == 0.   status 1   the winner flips at least one bit; its flips are
 *              applied.   status 2   no T has a candidate; nothing is flipped (a perfect code, n = 2^r - 1, never gets here).
 * out[R][C][6] int32 = status, pre_err (the weight of e over the n bits), post_err (the weight after the flips), nflip, erased (x_j == 0 after
 * the NaN map), pay_err (post_err restricted to the payload, the first K bits of the codeword, 1 <= K <= n).  A miscorrection is status 1 with
 * post_err > 0, an undetected error status 0 with pre_err > 0.
 * The payload stream (both pointers or neither): llr_out[R][C K] float32 and bits_out[R][C K] int8.  Payload bit i of codeword c is stream entry
 * u = c K + i (spread == 0) or u = i C + c (spread == 1: a bit interleaver over the run, which turns one failed inner word into isolated errors,
 * as vaeq_bch_outer's spread does).  An entry holds +1.0f / -1.0f for a decided 0 / 1 (the TX bit xor the final error bit) and the TX bit: the
 * stream is a valid [R][1][C K] input (w = 1, N = C K, t0 = 0) of every decoder above, which is the whole concatenation.
 * Workgroups of four waves, grid-stride over tiles of up to 32 consecutive codewords of a run (at most 2048 bits), gathered by all four and then
 * decoded one wave per codeword; the columns, a 2^r syndrome -> position table, the tile and its part of the stream in LDS (under 24 KiB).
 * Integers and a fixed order of float32 additions: two calls give identical bits.
 * Refusals, all before any HIP call and in vaeq_ldpc_decode's order: R == 0 is VAEQ_OK (its pointers may be NULL); a NULL cols_host, llr, bits or
 * out, or exactly one of llr_out and bits_out, is VAEQ_ERR_NULL, before any shape rule; then VAEQ_ERR_SHAPE for the tensor rules of the LDPC calls
 * (R < 0, C < 1, N < 1, N > 0x3fffffff, w outside 1 .. 64, t0 < 0, t0 > N), depth outside 0 .. C, n outside 3 .. 256, r outside 2 .. 10, p outside
 * 0 .. min(6, n), K outside 1 .. n, spread outside 0 .. 1, that depth's fit rule (t0 w + C n > N w, or t0 + C ceil(n / w) > N), R C > 0x7fffffff, and
 * C K > 0x3fffffff when a stream is asked for; last for the table: a column below 1 or >= 2^r, or one that occurs twice. */
int vaeq_chase_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t n, int32_t r, const int32_t *cols_host,
                      const float *llr, const int8_t *bits, int32_t p, int32_t K, int32_t spread, int32_t *out, float *llr_out,
                      int8_t *bits_out, void *stream);

/* Soft-decision turbo product codes: a Chase-Pyndiah soft-in / soft-out decoder of a product code whose rows and columns are words of two
 * single-error-correcting codes, iterated rows / columns, as the 100G soft-decision FEC of coherent optics decoded its extended-Hamming product
 * codes (no reference counterpart).  Unlike the float32 min-sum LDPC decoder it is NOT invariant to a common factor on the LLRs: it mixes them
 * with a beta given in absolute units (times scale), so it shows what an equalizer's noise-variance estimate costs behind the FEC.
 * The code: a block is an array of n1 x n2 bits, n = n1 n2.  Every row is a word of the row code cols2_host[n2] (columns of r2 bits), every
 * column a word of the column code cols1_host[n1] (columns of r1 bits); both are vaeq_chase_decode tables (host memory, validated on every call,
 * by value to the kernel) under its rules: n1, n2 in 3 .. 256, r1, r2 in 2 .. 10, the columns distinct, non-zero and below 2^r.
 * The tensors llr[R][w][N] / bits[R][w][N] and the bit-packed map are vaeq_ldpc_decode's with this n, C blocks per run: bit (a, b) of block c is
 * global bit g = c n + a n2 + b at symbol t0 + g / w, plane g % w, and t0 w + C n <= N w.  No interleaver option: a product code is its own.
 * No encoder: both codes are linear and the rule symmetric; it is stated on r, the LLR towards the transmitted bit, and acts there exactly as a
 * real decoder acts on a transmitted codeword -- except for inputs that are exactly zero, which a real decoder reads as bit 0 whatever was sent
 * and which here become a zero towards the transmitted bit (-0 against a TX bit 1, +0 otherwise; neither is < 0).
 * The rule, in integers and float32 so that a numpy model reproduces every bit:
 *   input      x_j = the LLR of bit j, a NaN mapped to +0;  r_j = bits_j ? -x_j : x_j, then clamped, min(max(r_j, -clip), clip), which also tames
 *              infinities.  pre_err counts (x_j < 0) xor bits_j, as every decoder here does; erased counts x_j == 0.
 *   state      W_j float32, +0 at the start.
 *   schedule   half-iterations h = 0 .. 2 iters - 1; an even h decodes all rows, an odd h all columns.  All words of a half-iteration are
 *              decided on the state before it (they own disjoint bits).  The soft input of a word is R_j = r_j + alpha_h W_j: one float32
 *              multiplication, then one float32 addition, not fused.
 *   one word   of length n' and table cols, as vaeq_chase_decode with a_j = |R_j| and e_j = (R_j < 0): s0 the xor of the columns with e_j = 1,
 *              the p least reliable positions by (a_j, j), the test patterns T = 0 .. 2^p - 1, their candidates, flip sets Phi_T and metrics
 *              m_T exactly as there, in the same order of additions; the winner D is the smallest (m_T, T); d_j = e_j xor [j in Phi_D].
 *              Status 0: s0 == 0.  Status 1: the winner flips.  Status 2: no candidate; then d_j = e_j and W'_j = +0 for the whole word.
 *   soft out   max-log, Pyndiah, per position j of a word of status 0 / 1: m_C(j) = the minimum of m_T over the candidates with j in the
 *              symmetric difference of Phi_T and Phi_D (a plain minimum: no order, no tie-break; candidates equal to D as a set compete
 *              nowhere).  With such a candidate: Delta = m_C(j) - m_D, one float32 subtraction, never negative; L_j = d_j ? -Delta : Delta;
 *              W'_j = L_j - R_j, one float32 subtraction.  Without one: W'_j = d_j ? -beta : beta with beta = fl(beta_h scale_r) where that
 *              product is > 0 (a NaN, a zero and a negative product give +0), at most clip; nbeta counts these positions.  Then W'_j is
 *              clamped, min(max(W'_j, -clip), clip), and replaces W_j.  Putting the extrinsic value of a position without a competitor at
 *              +-beta is a choice: it is the form used in most work after Pyndiah 1998, not the only one.
 *   stop       after half-iteration h the decisions d of the whole block are tested: if no word of h had status 2 and every word of the OTHER
 *              direction has a zero syndrome on d, decoding stops, ok = 1.  The test also runs after the last half-iteration.  A clean block
 *              costs one half-iteration.
 * out[R][C][8] int32, the first five in vaeq_staircase_decode's layout: iters (half-iterations executed), ok, post_err (the weight of the final
 * d), pre_err, erased, pay_err (final errors among rows < K1 and columns < K2, 1 <= K1 <= n1, 1 <= K2 <= n2), nstat2 (status-2 words over all
 * executed half-iterations), nbeta.
 * Nullable: llr_out[R][C n] float32 and bits_out[R][C n] int8 (both or neither), a stream as vaeq_chase_decode's -- +1.0f / -1.0f for the
 * decided bit (the TX bit xor the final d) and the TX bit, block after block in bit order, a valid [R][1][C n] input of every decoder here;
 * ext[R][C][n] float32, W after the last executed half-iteration, as it stands; half_err[R][C][2 iters] int32, the weight of d after each
 * executed half-iteration, -1 behind the stop.  scale[R] float32 in DEVICE memory, nullable = 1.0f; alpha_host[2 iters], beta_host[2 iters] in
 * host memory.
 * Bounds: p in 0 .. min(6, n1, n2), iters in 1 .. 16, every alpha_h finite in [0, 16], every beta_h finite and >= 0, clip finite in (0, 2^96].
 * Under them no infinity and no NaN arises anywhere: |r|, |W| and beta are at most clip, so |R| <= 17 clip, a metric adds at most 7 of those and
 * every difference stays below 2^105.
 * One workgroup per block in flight, grid-stride; r, W and a byte of TX bit and decision per bit stay in LDS for all half-iterations, the rows at
 * the odd stride n2 | 1; one wave per word, the competitors by LDS atomic minima on the metrics' bit patterns (order-free: two calls give
 * identical bits).  16 waves where n > 4096, else 4.  vaeq_tpc_lds_bytes(n1, r1, n2, r2) = 8 n1 (n2 | 1) (r and W) + n1 (n2 | 1) padded to a
 * word (the bytes) + 4 waves max(n1, n2) (a competitor array per wave) + 2 (n1 + n2) padded to a word (the columns) + 2 (2^r1 + 2^r2) (syndrome
 * -> position), the kernel's dynamic LDS, at most 156 KiB: with the kernel's static counters (under 1 KiB) that fits the 160 KiB of a CU.  The
 * extended (128, 120)^2 block holds 158 336 bytes.  That call returns VAEQ_ERR_SHAPE outside the ranges of n1, r1, n2, r2 and VAEQ_ERR_LDS above
 * the bound.
 * Refusals, all before any HIP call and in vaeq_chase_decode's order: R == 0 is VAEQ_OK (its pointers may be NULL); a NULL cols1_host,
 * cols2_host, llr, bits, alpha_host, beta_host or out, or exactly one of llr_out and bits_out, is VAEQ_ERR_NULL, before any shape rule; then
 * VAEQ_ERR_SHAPE for the tensor rules of the LDPC calls (R < 0, C < 1, N < 1, N > 0x3fffffff, w outside 1 .. 64, t0 < 0, t0 > N), the ranges
 * above, K1 outside 1 .. n1, K2 outside 1 .. n2, the fit rule (t0 w + C n > N w; C n stays below 2^47), R C > 0x7fffffff, and C n > 0x3fffffff
 * when a stream is asked for; then VAEQ_ERR_LDS for a state above the bound; last VAEQ_ERR_SHAPE for the two tables, cols1_host first: a column
 * below 1 or >= 2^r, or one that occurs twice. */
int vaeq_tpc_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0,
                    int32_t n1, int32_t r1, const int32_t *cols1_host, int32_t n2, int32_t r2, const int32_t *cols2_host,
                    const float *llr, const int8_t *bits, int32_t p, int32_t iters,
                    const float *alpha_host, const float *beta_host, const float *scale, float clip,
                    int32_t K1, int32_t K2, int32_t *out, float *llr_out, int8_t *bits_out, float *ext, int32_t *half_err, void *stream);
int64_t vaeq_tpc_lds_bytes(int32_t n1, int32_t r1, int32_t n2, int32_t r2);

/* The two Chase decoders over (extended) double-error-correcting BCH words, the components of the soft-decision product codes that 100G line
 * cards shipped and of today's open-FEC family: minimum distance 6 with the parity bit, against 4 of an extended Hamming word (no reference
 * counterpart).  Everything that is not said here is vaeq_chase_decode's and vaeq_tpc_decode's, word for word.
 * The code: vaeq_bch_outer's narrow-sense primitive binary BCH code over GF(2^m) with designed correction t = 2 -- the same polynomials, position
 * p belongs to alpha^p -- shortened to n_i inner bits, followed, where ext == 1, by one overall parity bit at position u = n_i: n = n_i + ext.
 * m in 4 .. 8, parity(m, 2) = 2 m < n_i <= 2^m - 1, so n <= 256; k = n_i - 2 m.  m = 7, n = 128, ext = 1 is the extended (128, 113) word, m = 8,
 * n = 256, ext = 1 the (256, 239) word.  Only t = 2: t >= 3 has no closed-form locator of this size and is out of scope.
 * The rule for one word, in the place of vaeq_chase_decode's lines "patterns" and "metric"; input, positions (the parity position takes part
 * like any other), winner, the three statuses, out[R][C][6], the payload stream, depth, spread and K are that call's:
 *   patterns   T = 0 .. 2^p - 1:  F_T = { l_i : bit i of T };  x = e xor F_T.  The inner part of x, its positions below n_i, is decided by
 *              vaeq_bch_outer's rule with t = 2 and n_o = n_i: status 0 gives V = {}; status 1 gives V, the unique set of one or two positions
 *              below n_i with the same S_1 .. S_4; status 2: T has no candidate.  If ext, u is flipped iff the weight of x over all n positions
 *              plus |V| is odd.  The candidate flips Phi_T = F_T delta V delta {u if flipped} (symmetric differences): e xor Phi_T is a codeword
 *              of the extended code, and |Phi_T| <= p + 3.
 *   metric     of a candidate: from +0.0f, add a_j over Phi_T one float32 addition at a time -- first its members among l_0 .. l_(p-1) in
 *              ascending i, then the others in ascending position (at most three; u, the largest position, last).  The metric is a function
 *              of the set alone.  (Predicated additions of +0.0f are the same sum, as above.)
 * (In closed form: S_1 = S_3 = 0: V = {}.  S_1 = 0 alone: no candidate.  S_3 = S_1^3: V = {log S_1}.  Otherwise V = {log(S_1 y), log(S_1 y +
 * S_1)} for a root y of y^2 + y = (S_3 + S_1^3) / S_1^3, no candidate where there is none.  A position >= n_i: no candidate.)
 * Status 0 is the case exactly when S_1 = S_3 = 0 and, if ext, the weight of e is even; the code is not perfect, so status 2 is reached at full length too.
 * vaeq_chase_bch_decode is vaeq_chase_decode with (m, n, ext) in the place of (n, r, cols_host): the same kernel body, the exp, log and
 * half-solve tables of GF(2^m) (3 2^m uint16) built in LDS in the place of the columns, and lane T decides pattern T by the closed form.
 * Refusals, all before any HIP call and in vaeq_chase_decode's order: R == 0 is VAEQ_OK; a NULL llr, bits or out, or exactly one of llr_out and
 * bits_out, is VAEQ_ERR_NULL; then VAEQ_ERR_SHAPE for the tensor rules, depth outside 0 .. C, m outside 4 .. 8, ext outside 0 .. 1, n - ext
 * outside 2 m + 1 .. 2^m - 1, p outside 0 .. min(6, n), K outside 1 .. n, spread outside 0 .. 1, the fit rule, R C > 0x7fffffff and C K >
 * 0x3fffffff when a stream is asked for. */
int vaeq_chase_bch_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0, int32_t depth, int32_t m, int32_t n, int32_t ext,
                          const float *llr, const int8_t *bits, int32_t p, int32_t K, int32_t spread, int32_t *out, float *llr_out,
                          int8_t *bits_out, void *stream);

/* vaeq_tpc_decode over two such codes: the column code (m1, n1, ext1) and the row code (m2, n2, ext2), which may differ in all three.  The rule is
 * vaeq_tpc_decode's word for word with "one word" the rule above; the soft input, the competitors (a candidate competes at j where j lies in the
 * symmetric difference of Phi_T and Phi_D; a plain minimum; beta where none competes), the clamps, the schedules, the counters, the stream, ext
 * and half_err are unchanged.  The stop test asks that no word of h had status 2 and that every word of the other direction has S_1 = S_3 = 0
 * on d and, if that code is extended, even weight.
 * Bounds as there.  A metric now adds at most 9 magnitudes (p + 3) of at most 17 clip, so with clip <= 2^96 every metric stays below 2^104 and
 * every difference below 2^105: no infinity and no NaN arises.
 * The same kernel body; a lane's competitor walk takes at most p + 5 places: the listed positions, its own up to two unlisted located
 * positions, the winner's, and the parity position.  vaeq_tpc_bch_lds_bytes(m1, n1, ext1, m2, n2, ext2) = 8 n1 (n2 | 1) + n1 (n2 | 1) padded
 * to a word + 4 waves max(n1, n2) + 6 2^m1 + (6 2^m2 if m2 != m1: one field, one set of tables), under the same bound of 156 KiB.  The extended
 * (128, 113)^2 block holds 157 568 bytes.  The (256, 239)^2 block does not fit -- 9 bytes per bit are 590 KB -- and is out of scope: it needs a
 * state outside LDS or a narrower one.  Also out of scope: a product of one Hamming and one BCH component, braided or staircase-shaped soft
 * decoding, a fixed-point form, an encoder.  That call returns VAEQ_ERR_SHAPE outside the envelope of either code and VAEQ_ERR_LDS above the bound.
 * Refusals, all before any HIP call and in vaeq_tpc_decode's order: R == 0 is VAEQ_OK; a NULL llr, bits, alpha_host, beta_host or out, or
 * exactly one of llr_out and bits_out, is VAEQ_ERR_NULL; then VAEQ_ERR_SHAPE for the tensor rules, the envelope of either code (as above), p
 * outside 0 .. min(6, n1, n2), iters, clip, the schedules, K1 outside 1 .. n1, K2 outside 1 .. n2, the fit rule, R C > 0x7fffffff, and C n >
 * 0x3fffffff when a stream is asked for; last VAEQ_ERR_LDS for a state above the bound. */
int vaeq_tpc_bch_decode(int32_t R, int32_t C, int64_t N, int32_t w, int64_t t0,
                        int32_t m1, int32_t n1, int32_t ext1, int32_t m2, int32_t n2, int32_t ext2,
                        const float *llr, const int8_t *bits, int32_t p, int32_t iters,
                        const float *alpha_host, const float *beta_host, const float *scale, float clip,
                        int32_t K1, int32_t K2, int32_t *out, float *llr_out, int8_t *bits_out, float *ext, int32_t *half_err, void *stream);
int64_t vaeq_tpc_bch_lds_bytes(int32_t m1, int32_t n1, int32_t ext1, int32_t m2, int32_t n2, int32_t ext2);

int vaeq_version(void);
const char *vaeq_strerror(int code);

/* Measurement helpers (no reference counterpart; SURVEY 8d asks for them).
 * vaeq_last_kernel: name of the kernel instantiation the calling thread's most recent vaeq_dp_train / vaeq_awgn_train / vaeq_cma / vaeq_cpe /
 * vaeq_nn_train / vaeq_nn_forward / vaeq_nn_validate / vaeq_nn_enc_forward / vaeq_nn_enc_backward / any *_bwd_x / vaeq_nn_enc_backward_x launched (as a profiler prints it, e.g. "vaeq::dp_wave_kernel<25, 8, 100, true, 1, 1, 0>" or "vaeq::cma_kernel<true, false>"), copied into
 * buf[len] -- bench.py names its roofline kernel from this, the tests check which vaeq_cma instantiation a shape reaches.
 * vaeq_stream_copy: dst[bytes] = src[bytes] with a plain 16-byte grid-stride copy kernel (bytes and both pointers multiples of 16): the
 * measured HBM copy bandwidth that stands next to the 8 TB/s spec peak in the roofline. */
int vaeq_last_kernel(char *buf, int32_t len);
int vaeq_stream_copy(void *dst, const void *src, int64_t bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VAEQ_H */
