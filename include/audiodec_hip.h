/*
 * audiodec_hip.h -- C ABI of libaudiodec_hip.so: the AudioDec streaming hot path on MI355X (gfx950).
 *
 * The reference (facebookresearch/AudioDec) has no native layer: its hot path is PyTorch module
 * methods.  This header is the FFI a maintainer would bind in their place (ctypes stub in
 * INTEGRATION.md); every entry point names the reference method(s) it replaces.
 *
 * Conventions
 *   - the matrix-core conv kernel keeps split-tile partial sums in a scratch workspace: a program owns
 *     one (allocated in adk_program_create); op-level adk_causal_conv uses a per-host-thread one that
 *     is allocated on that thread's first call
 *   - all data pointers are DEVICE pointers (fp32 unless stated); `stream` is a hipStream_t passed
 *     as void*; calls enqueue work on that stream and return without synchronising
 *   - return value: 0 = ADK_OK, negative = error (text via adk_last_error(), thread-local)
 *   - no hidden device allocation in step/op calls; a handle may be used by one host thread at a
 *     time, different handles concurrently (reference threading model: bin/stream.py:212-239)
 *   - devices: every call runs on the HIP device that OWNS its buffers, whatever device the calling thread has
 *     current (the reference's --tx_cuda / --rx_cuda put the two halves on different GPUs, demoStream.py:33-40):
 *     a program is bound to the device of its arena at adk_program_create; op-level calls look the device up from
 *     their output pointer; the scratch workspace and the sticky flag word are per device
 *
 * Data layout ("rings")
 *   Every stateful conv input lives in a ring of channel-last rows: ring[b][r][c], r in [0,rows),
 *   one row = one time step of `channels` floats.  The reference's per-layer `pad_buffer`
 *   (layers/conv_layer.py:144-146,153-156) is the `hist` rows in front of the cursor; producers write
 *   new rows at the cursor, consumers read [cursor-hist, cursor+T); nothing is ever copied or
 *   shifted.  The ring stores the RAW (pre-activation) signal; the consumer's input activation
 *   (ELU / LeakyReLU) is applied while the tile is staged on chip.
 */
#ifndef AUDIODEC_HIP_H
#define AUDIODEC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADK_ABI_VERSION 14

enum { ADK_OK = 0, ADK_ERR_ARG = -1, ADK_ERR_SHAPE = -2, ADK_ERR_HIP = -3, ADK_ERR_STATE = -4 };

/* activations: layers/activation_function.py:18-22 -> torch.nn.{ELU,LeakyReLU,Tanh} */
enum { ADK_ACT_NONE = 0, ADK_ACT_ELU = 1, ADK_ACT_LEAKY = 2, ADK_ACT_TANH = 3 };

/* kernel selection for adk_causal_conv (ADK_IMPL_AUTO in production; others for tests/benchmarks) */
enum { ADK_IMPL_AUTO = 0, ADK_IMPL_DIRECT = 1, ADK_IMPL_MFMA = 2 /* stream-K implicit GEMM */, ADK_IMPL_MFMA_ROWS = 3 /* rows-in-LDS */,
       /* Opt-in split-precision kernels: every f32 operand is carried as f16 hi + f16 lo/2048 and a product sum is
          formed from three f16 MFMAs (hi*hi, hi*lo, lo*hi) with f32 accumulation -- measured error vs fp64 is
          below that of the f32 MFMA chain (profiles/r1_f16_split_probe.txt).  w_frag must then hold the
          adk_pack_weights_split16 layout.  |operand| > 65504 (-> non-finite outputs) raises device flag bit 3.
          SPLIT16 picks between the rows-in-LDS and the stream-K variant like AUTO does; the other two force one. */
       ADK_IMPL_SPLIT16 = 4, ADK_IMPL_SPLIT16_ROWS = 5, ADK_IMPL_SPLIT16_SK = 6,
       /* the streaming kernel of the last up-sampling stage (fused activation -> ConvTranspose1d 64 -> Cout, s*Cout <= 96,
          + bias; HiFiGAN.py:285-289): SPLIT16 picks it for that layer shape, this value forces it */
       ADK_IMPL_SPLIT16_UP = 7 };

const char* adk_last_error(void);
int adk_abi_version(void);
/* sticky device-side flags since the last call (bit 0: adk_rvq_lookup saw an out-of-range index,
 * where F.embedding would raise; bit 1: a stream-K conv workgroup gave up waiting for another workgroup's
 * partial tile -- results of that launch are invalid; bit 2: adk_codes_pack saw an index that
 * is not a code of its stage; bit 3: a split-f16 kernel produced a non-finite output -- an operand beyond the f16 range (|v| > 65504) or a
 * non-finite input; results of that launch are invalid); the value is the OR over every device the library
 * has launched on and every program on them (one sweep kernel per device over the pool the program words live in);
 * reading synchronises those devices and clears the words.  The Python facade turns a set bit
 * into an exception at its synchronisation points (audiodec_amd/native.py: raise_on_device_flags) */
int adk_debug_flags(int32_t* out);
/* tuning hook: force the stream-K conv tile config; -1 = heuristic (the default).  0: 128x64 (the split-f16 kernel only: the exact-f32
 * kernel has no such build and keeps its own choice), 2: 64x64, 4: 32x128.  ADK_ERR_ARG for any other id. */
int adk_set_conv_cfg(int32_t cfg);
/* tuning / test hook: named process-wide integer options, read at every launch decision.
 *   "chain_max_channels"  residual chains (adk_op_desc.chain) run as one launch only up to this many channels per group
 *                         (default 128 = every chain the kernel takes; 64: not the 128-channel ones; 0: never -- the ops of a
 *                         chain are then launched one by one, as with ADK_CHAIN=0).  State rings are compatible either way:
 *                         the value may change between two steps of a running program.
 *   "chain_min_blocks"    ... and only for launches of at least this many (stream, group) pairs (default 0: always.  Until round 4 the
 *                         default was 160 -- with the chain kernels of that time the per-op launches, which spread a stream's time tiles
 *                         over many CUs, were faster below it; now the chain is faster at every launch size: 1 stream 0.74 -> 0.71 ms per
 *                         frame, 48 streams 0.86 -> 0.77 ms, profiles/r4_few_streams.md)
 *   "rvq_rows"            rows per workgroup of the residual-VQ search when dim == 64, size == 1024 (csrc/rvq.hip, rvq_encode_v4): from
 *                         "rvq_v4_min" rows (default 192) on, 2 or 4 rows share a workgroup's code registers; 1 (default) = 2 up to 512
 *                         rows, 4 above; 0: the round-3 kernels at every row count.  Indices and zq are bit-identical either way.
 *   "rvq_v4_min"          see above
 *   "gv16_max_columns"    convs of at most this many columns (streams x steps per call) run as conv_gv16 (csrc/conv_mfma.hip: one wave per
 *                         32-row x 32-column output tile and K slice, no LDS) instead of the stream-K kernel; default 32, 0 = never.
 *                         Results of the two kernels agree to f32 round-off, not bit for bit.
 *   "conv_ou16", "conv_oc16", "conv_cin1w"   0: the op pairs these launches cover run as two launches again (defaults 1):
 *                         conv_out + the last up-sampler (csrc/conv_ou16.hip: f32 round-off against the two-launch
 *                         form), the last conv_out + the output conv (csrc/conv_oc16.hip), the encoder's ring write + its Cin = 1 conv
 *                         (csrc/conv_direct.hip: bit-identical).  A/B measurements and the tests that compare the two forms.
 *   "conv_rk16"           split-f16 convs of wide groups (>= 128 input channels per group, K 7 or 11, stride 1) whose taps share input rows
 *                         across the steps of a call run as conv_rk16 (csrc/conv_rk16.hip: whole 64 x 64 tiles, rows staged once in LDS,
 *                         no K split) instead of the stream-K kernel.  1 (default; the environment's ADK_CONV_RK16 sets another one):
 *                         launches of at least 192 tiles, i.e. that fill the chip; 2: every launch of the shape class (tests); 0: never.
 *                         The rings and shadow rings the two kernels leave are interchangeable, the value may change between two calls;
 *                         results agree to f32 round-off, not bit for bit.  adk_causal_conv_describe / adk_program_describe_op name the
 *                         launch "conv_sk16<rk16 64x64>".
 * ADK_ERR_ARG for an unknown name. */
int adk_set_option(const char* name, int32_t value);
/* Introspection of the stream-K launch schedule (pure host logic, no device needed; used by the CPU tests): a matrix-core conv
 * launch over `tiles` output tiles of `chunks` 64-deep K chunks each, allowed at most `cap` persistent workgroups (0: the library
 * default), runs plan[0] workgroups ("ranges").  plan[1] > 0: every tile is cut into plan[1] ranges (plan[1] == 2: the first takes
 * plan[3] chunks); plan[2] > 0: every range takes plan[2] whole tiles; both 0: tiles * chunks / plan[0] work units each, wherever
 * that cuts.  adk_streamk_range_start gives the first work unit (tile * chunks + chunk) of range r, r = plan[0]: one past the last;
 * -1 on a bad argument. */
int adk_streamk_plan(int64_t tiles, int32_t chunks, int32_t cap, int32_t* plan /* [4] */);
int64_t adk_streamk_range_start(int64_t tiles, int32_t chunks, const int32_t* plan, int32_t r);
/* Introspection of the residual-chain launch (csrc/conv_rb16.hip; pure host logic, no device needed): what a chain of `n_convs` convs
 * (A_0, B_0, A_1, ...: `channels` per group in and out, taps_a / taps_b taps, activation `act` in front of every conv, dilations[k] of conv k)
 * would run as for `batch` streams, `groups` groups and `steps` new time steps per call.  The plan comes out of the functions the launch
 * itself goes through.  plan[0] = 1: the chain kernel takes the call (0: the ops run one by one; the other words are 0), and then
 *   plan[1]  template arm: 1 32 ch weight ring | 2 32 ch two tiles, <= 128 workgroups | 3 32 ch three tiles K11 | 4 32 ch three tiles |
 *            5 32 ch four tiles | 6 64 ch weight ring | 7 64 ch two tiles, <= 128 workgroups | 8 64 ch three tiles | 9 64 ch four tiles |
 *            10 128 ch one stream, one tile | 11 128 ch two tiles | 12 128 ch two streams in one tile.  Every arm is built for the four
 *            tap sets (LeakyReLU 11/11, 7/7, 3/3; ELU 7/1)
 *   plan[2]  streams per workgroup        plan[3]  32-column tiles per wave        plan[4]  tiles of a full workgroup
 *   plan[5]  slots of the LDS weight ring plan[6]  1: at most 128 workgroups       plan[7]  1: L2 warm-up touches
 *   plan[8]  helper workgroups per XCD    plan[9]  convs whose weights they touch  plan[10] dynamic LDS bytes
 *   plan[11] computing workgroups         plan[12] workgroups launched             plan[13] 8-channel history pieces the arm can stage
 *   plan[14] pieces the longest history of the chain needs (<= plan[13])          plan[15] rows of that history
 * ADK_ERR_ARG: null pointer, n_convs not 2, 4, 6 or 8, or a count below 1. */
#define ADK_RB16_PLAN_WORDS 16
int adk_conv_rb16_plan(int32_t channels, int32_t taps_a, int32_t taps_b, int32_t act, const int32_t* dilations, int32_t n_convs,
                       int32_t batch, int32_t groups, int32_t steps, int32_t* plan /* [ADK_RB16_PLAN_WORDS] */);

/* A view of one ring for one call. */
typedef struct {
    float*  base;      /* stream b starts at base + b * rows * channels                            */
    int32_t rows;      /* ring length R                                                             */
    int32_t channels;  /* row length C (all groups)                                                 */
    int32_t cursor;    /* row of the first NEW time step of this call, 0 <= cursor < rows           */
    int32_t ch_off;    /* first channel this op touches                                             */
} adk_ring_view;

/*
 * One fused causal convolution:  replaces
 *   CausalConv1d.inference            layers/conv_layer.py:153-156  (up == 1)
 *   CausalConvTranspose1d.inference   layers/conv_layer.py:194-197  (up == stride s; polyphase form:
 *       taps = 2, cout_g = s*Cout, weight row (r*Cout+co) = [W[:,co,s+r] | W[:,co,r]])
 *   Conv1d1x1                         layers/conv_layer.py:28-32    (taps == 1, hist == 0)
 * plus the element-wise ops the reference runs around them: input activation, bias, residual add
 * (residual_unit.py:78-81, residual_block.py:99-105), output activation (HiFiGAN.py:294-296).
 *
 * For stream b, output step t in [0, t_out), GEMM row m in [0, groups*cout_g), g = m / cout_g:
 *   acc = bias[m] + sum_{j<taps} sum_{ci<cin_g}
 *           w[m][j*cin_g + ci] * act_in( in[b][(in.cursor - hist + t*stride + j*dilation) mod R][in.ch_off + g*in_group_stride + ci] )
 *   acc += res[b][(res.cursor + t) mod R][res.ch_off + g*res_group_stride + (m mod cout_g)]     (if res.base)
 *   out[b][(out.cursor + t*up + m / cout_real) mod R][out.ch_off + m mod cout_real] = act_out(acc)
 */
typedef struct {
    int32_t cin_g, cout_g, groups;       /* per-group channels                                       */
    int32_t taps, stride, dilation;      /* stride = input rows per output step                      */
    int32_t hist;                        /* history rows in front of in.cursor: (taps-1)*dilation    */
    int32_t up, cout_real;               /* up == 1: cout_real = groups*cout_g; transposed: see above */
    int32_t in_group_stride;             /* 0 when all groups read the same channels (x.repeat, multi_fusion.py:134) */
    int32_t res_group_stride;
    int32_t act_in;  float act_in_slope;
    int32_t act_out;
    const float* w;                      /* [groups*cout_g][taps*cin_g], tap-major / channel-minor; may be NULL when
                                            w_frag is given and the MFMA kernel is taken             */
    const float* w_frag;                 /* the same weights in MFMA-fragment order (adk_pack_weights_mfma) or NULL:
                                            without it only the VALU kernel can run                  */
    const float* bias;                   /* [groups*cout_g] or NULL                                  */
} adk_conv_desc;

/* Re-pack row-major conv weights [groups*cout_g][ktot] for the matrix-core kernel:
 * out[g][m-tile of 32][k-group of 8][lane 0..63][4] with lane (i = lane&31, h = lane>>5) holding
 * W[32*mt + i][8*kg + 4*h + 0..3]; rows beyond cout_g and the K tail (K is padded to a multiple
 * of 64) are zero.  out needs
 * adk_packed_weight_floats(groups, cout_g, ktot) floats; ktot % 8 == 0.  Done once at load time. */
int64_t adk_packed_weight_floats(int32_t groups, int32_t cout_g, int32_t ktot);
int adk_pack_weights_mfma(const float* w, float* out, int32_t groups, int32_t cout_g, int32_t ktot, void* stream);
/* Split-f16 fragment order for ADK_IMPL_*_SPLIT16: out[g][m-tile of 32][16-k chunk][hi | lo][lane 0..63][8 x f16]
 * with lane (i = lane&31, h = lane>>5) holding W[32*mt + i][16*chunk + 8*h + 0..7], hi = f16(W),
 * lo = f16((W - hi) * 2048); rows beyond cout_g are zero.  ktot % 16 == 0; out needs
 * adk_packed_weight_floats_split16(groups, cout_g, ktot) floats (= 32*mt32 * ktot per group). */
int64_t adk_packed_weight_floats_split16(int32_t groups, int32_t cout_g, int32_t ktot);
int adk_pack_weights_split16(const float* w, float* out, int32_t groups, int32_t cout_g, int32_t ktot, void* stream);

int adk_causal_conv(const adk_conv_desc* d, adk_ring_view in, adk_ring_view out, adk_ring_view res,
                    int32_t batch, int32_t t_out, int32_t impl, void* stream);
/* name of the kernel the call above would launch (e.g. "conv_sk16<128x64>"), nothing is launched: for profiles and
 * for tests that must know which kernel they exercised */
int adk_causal_conv_describe(const adk_conv_desc* d, adk_ring_view in, adk_ring_view out, adk_ring_view res,
                             int32_t batch, int32_t t_out, int32_t impl, char* buf, int32_t n);
/* timing aid (bench.py, tools): `iters` back-to-back launches of the call above on `stream`, bracketed by HIP events recorded
 * on that stream; synchronises; *avg_us = average microseconds per launch (no host language in the loop) */
int adk_causal_conv_time(const adk_conv_desc* d, adk_ring_view in, adk_ring_view out, adk_ring_view res,
                         int32_t batch, int32_t t_out, int32_t impl, int32_t iters, void* stream, float* avg_us);

/*
 * Copy caller rows into a ring, optionally normalising: ring row = (src - mean) / scale.
 * Replaces the torch.cat of new samples onto the state (conv_layer.py:154) for the first layer and
 * HiFiGAN StreamGenerator.decode_norm (models/vocoder/HiFiGAN.py:276-279; true division).
 * src is [batch][t][channels] contiguous.
 */
int adk_ring_write(const float* src, adk_ring_view ring, const float* mean, const float* scale,
                   int32_t batch, int32_t t, void* stream);

/*
 * Residual VQ encode: replaces ResidualVQ.forward_index(flatten_idx=True) over
 * VectorQuantize.forward_index (layers/vq_module.py:136-149, 90-104) for n_rows = B*T rows.
 *   z      [n_rows][dim]            (channel-last latent, i.e. Quantizer.encode's z.transpose(2,1))
 *   embed  [n_q][dim][size]         the reference's `embed` buffers (codes are columns)
 *   enorm  [n_q][size]              embed.pow(2).sum(0) (vq_module.py:96), computed once at load
 *   idx    [n_q][n_rows] int64      emitted index = code + size*stage (vq_module.py:145-146)
 *   zq     [n_rows][dim] or NULL    sum of the straight-through quantised vectors (quantized_out)
 * Arithmetic per stage follows the reference literally: dist = (|r|^2 - (2r).E) + |E|^2, argmax of
 * -dist with lowest index on ties, q' = r + (q - r), r <- r - q'.
 */
int adk_rvq_encode(const float* z, const float* embed, const float* enorm, int64_t* idx, float* zq,
                   int32_t n_rows, int32_t n_q, int32_t dim, int32_t size, void* stream);

/*
 * Residual VQ lookup: replaces ResidualVQ.lookup (layers/vq_module.py:159-161).
 *   idx [n_q][n_rows] int64 (global indices 0..n_q*size-1), codebook [n_q*size][dim]
 *   zq  [n_rows][dim] = sum over stages, stage 0 first
 * An out-of-range index reads code 0 and raises bit 0 of adk_debug_flags().
 */
int adk_rvq_lookup(const int64_t* idx, const float* codebook, float* zq,
                   int32_t n_rows, int32_t n_q, int32_t dim, int32_t n_codes, void* stream);

/*
 * Residual VQ statistics: the per-stage commitment loss and code histogram of ResidualVQ.forward / VectorQuantize.forward in
 * eval mode (layers/vq_module.py:61-88, 119-134), for codes adk_rvq_encode emitted.
 *   z        [n_rows][dim]           the latent rows given to adk_rvq_encode
 *   codebook [n_q*size][dim]         row-major codes (the adk_rvq_lookup layout)
 *   idx      [n_q][n_rows] int64     emitted indices, stage s in [size*s, size*(s+1))
 * Each row's residual chain is rebuilt with adk_rvq_encode's f32 step (q' = r + (q - r), r <- r - q'), so r_s is the residual
 * stage s searched.  The call FOLDS into a caller-owned accumulator on the device (zero it to start; nothing is cleared here):
 *   counts [n_q*size] int64   += the code histogram of every stage (global index order)
 *   sse    [n_q] double       += sum over rows and components of (q_s - r_s)^2 (f32 difference and square, f64 sum)
 *   rows   [1] int64          += n_rows
 * vqloss [n_q] f32 (or NULL) = sse / (rows * dim) and perplexity [n_q] f32 (or NULL) = exp(-sum_k p_k log(p_k + 1e-10)) with
 * p_k = count_k / rows in f32, both from the totals AFTER this call's fold (NaN while rows == 0).  n_rows == 0 folds nothing and
 * only writes what is asked for.  workspace: adk_rvq_stats_workspace_bytes(n_rows, n_q) bytes, 8-byte aligned, any contents,
 * unused once the call's work has finished (NULL when that size is 0).  Bitwise reproducible: float sums go through
 * per-workgroup slabs in a fixed order.  Calls on one accumulator must be ordered (one stream).  An index outside its stage
 * counts nothing, reads that stage's first code and raises bit 0 of adk_debug_flags().  Limits: dim <= 128, n_q <= 16,
 * n_q*size < 2^31.  Every argument is checked before any HIP call (ADK_ERR_ARG).
 */
int64_t adk_rvq_stats_workspace_bytes(int32_t n_rows, int32_t n_q);
int adk_rvq_stats(const float* z, const float* codebook, const int64_t* idx, int32_t n_rows, int32_t n_q, int32_t dim,
                  int32_t size, int64_t* counts, double* sse, int64_t* rows, void* workspace, float* vqloss,
                  float* perplexity, void* stream);

/*
 * Residual VQ codebook update: the training branch of VectorQuantize.forward (layers/vq_module.py:74-80) for every stage of one
 * ResidualVQ.forward, from the latents z [n_rows][dim] and the emitted indices idx [n_q][n_rows] (stage offset included) -- what
 * adk_rvq_stats takes.  The residual entering stage s is rebuilt with adk_rvq_encode's f32 step from the OLD embed of every stage
 * (the reference looks the codes up before a stage rewrites them), then per stage, all in f32 round-to-nearest, nothing contracted,
 * with (float)decay and (float)(1.0 - decay):
 *   cluster_size <- decay*cluster_size + (1-decay)*count_k
 *   embed_avg    <- decay*embed_avg + (1-decay)*sum_{rows with code k} r_s       (the sum in f64, ascending row order, rounded once)
 *   S = sum_k cluster_size (f64, fixed order);  smoothed_k = (cluster_size_k + eps) / (S + size*eps) * S
 *   embed[:,k] = embed_avg[:,k] / smoothed_k
 *   embed        [n_q][dim][size]   read (old codes), then overwritten
 *   enorm        [n_q][size]        overwritten: |embed[:,k]|^2
 *   codebook     [n_q*size][dim]    row-major twin of the new embed, overwritten; may be NULL
 *   cluster_size [n_q][size], embed_avg [n_q][dim][size]   in/out
 * so adk_rvq_encode / adk_rvq_lookup can follow on the same stream.  A code no row chose only decays (its quotient may grow large, as
 * in the reference).  Bitwise reproducible and independent of the launch geometry (adk_set_option("rvq_ema_chunk_rows", n) moves it;
 * 0 = default): no floating-point atomics.  An index outside its stage counts nothing, sums nothing, reads that stage's first code
 * for the rest of the row's chain and raises bit 0 of adk_debug_flags().  workspace: adk_rvq_ema_workspace_bytes(...) bytes, 8-byte
 * aligned, any contents, unused once the call's work has finished.  A stage whose cluster sizes are all zero and none of whose
 * rows carries a code of that stage (every one flagged through bit 0) has S = 0: its smoothed sizes and embed become NaN, as the
 * reference's would on an empty batch.  Limits: n_rows > 0, dim <= 128, n_q <= 16, n_q*size <= 2^28, 0 <= decay < 1, eps > 0.  Every argument is checked before any HIP call (ADK_ERR_ARG).
 */
int64_t adk_rvq_ema_workspace_bytes(int32_t n_rows, int32_t n_q, int32_t dim, int32_t size);
int adk_rvq_ema_update(const float* z, const int64_t* idx, int32_t n_rows, int32_t n_q, int32_t dim, int32_t size,
                       double decay, double eps, float* embed, float* enorm, float* codebook, float* cluster_size,
                       float* embed_avg, void* workspace, void* stream);

/*
 * Log-mel spectrogram and mel L1 distance: MelSpectrogram.forward and one resolution of MultiMelSpectrogramLoss.forward
 * (losses/mel_loss.py:19-156), with torch.stft's defaults as the reference calls it: center=True with reflect padding of n_fft/2
 * on each side, no normalisation, a one-sided spectrum of n_fft/2 + 1 bins, 1 + n_samples/hop frames.
 *   x / a / b   [n_signals][n_samples]     signals, contiguous
 *   window      [win_length]               the analysis window (torch.hann_window(win_length)), centred in n_fft with
 *                                          (n_fft - win_length)/2 zeros on the left, as torch.stft pads it
 *   fb_range    [n_mels][3] int32          filter m: first bin, bin count, offset of its weights in fb_weight
 *   fb_weight   [n_weights]                the nonzero weights of melmat, filter by filter, in bin order
 *   amp = sqrt(max(re^2 + im^2, eps)); mel = max(sum_k amp[k] w_m[k], eps); log_base 0 = natural log, 2 = log2, 10 = log10.
 * adk_logmel writes out [n_signals][n_mels][frames] f32.  adk_mel_distance FOLDS sum |logmel(a) - logmel(b)| (f32 difference,
 * f64 sum) into a caller-owned accumulator on the device (zero it to start; nothing is cleared here):
 *   sum [1] double += the sum;  count [1] int64 += n_signals * n_mels * frames
 * and, if loss is not NULL, writes loss [1] f32 = sum / count from the totals after this call's fold (NaN while count == 0).
 * n_signals == 0 folds nothing.  workspace: adk_mel_workspace_bytes(n_signals, n_samples, n_fft, hop) bytes, 8-byte aligned,
 * any contents (NULL when that size is 0).  The log-mels are never written to memory; the sum goes through per-workgroup f64
 * slabs and a fixed-order finalize launch, so it is bitwise reproducible.  Calls on one accumulator must be ordered (one stream).
 * NaN input gives NaN output, as in the reference.  Limits: n_fft a power of two in [256, 4096], 0 < win_length <= n_fft,
 * hop > 0, n_samples > n_fft/2 (the reflect padding; torch raises too), 0 < n_mels <= 256, log_base in {0, 2, 10}.  Every
 * argument is checked before any HIP call (ADK_ERR_ARG).  No allocation, no synchronisation.
 */
int64_t adk_mel_workspace_bytes(int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop);
int adk_logmel(const float* x, int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop, const float* window,
               int32_t win_length, const int32_t* fb_range, const float* fb_weight, int32_t n_weights, int32_t n_mels,
               int32_t log_base, float eps, float* out, void* stream);
int adk_mel_distance(const float* a, const float* b, int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop,
                     const float* window, int32_t win_length, const int32_t* fb_range, const float* fb_weight, int32_t n_weights,
                     int32_t n_mels, int32_t log_base, float eps, double* sum, int64_t* count, void* workspace, float* loss,
                     void* stream);

/*
 * Mel-spectrogram loss, backward: the vector-Jacobian products of the two operations above with respect to the signal, as
 * torch's autograd defines them for losses/mel_loss.py:84-94 (clamp passes the gradient where its input >= eps).  The arguments
 * shared with adk_logmel mean the same; in addition the mel filters transposed, one contiguous filter range per bin:
 *   tb_range    [n_fft/2 + 1][3] int32     bin k: first filter, filter count, offset of its weights in tb_weight
 *   tb_weight   [n_tweights]               melmat[first .. first + count)[k], bin by bin, in filter order (inner zeros kept)
 * adk_logmel_vjp: g [n_signals][n_mels][frames] f32 is the gradient of adk_logmel's out; grad_x [n_signals][n_samples] f32
 * = sum over out of g d out / d x.  adk_mel_distance_grad: grad_a [n_signals][n_samples] = the gradient with respect to a of
 * c sum |logmel(a) - logmel(b)|, c = (float)(scale * upstream[0]); upstream is a device pointer to one f32, read on the device.
 * It is the same product with g = sign(logmel(a) - logmel(b)) c, the log-mels and their f32 difference being exactly those
 * adk_mel_distance and adk_logmel compute, and sign(0) = 0.  For the mean over one resolution, scale = 1 / count.
 * Each frame's forward is recomputed (no spectra are kept); its windowed gradient goes to workspace
 * [n_signals][frames][n_fft] f32 = adk_mel_grad_workspace_bytes(n_signals, n_samples, n_fft, hop) bytes, 4-byte aligned, any
 * contents; a second launch gathers every sample's contributions through the reflect padding in ascending frame order.  No float
 * atomics: bitwise reproducible.  grad_x / grad_a is fully written (a sample no frame reaches gets 0).  n_signals == 0 is a
 * no-op.  Same limits as adk_logmel; every argument is checked before any HIP call (ADK_ERR_ARG).  No allocation, no
 * synchronisation.
 */
int64_t adk_mel_grad_workspace_bytes(int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop);
int adk_logmel_vjp(const float* x, const float* g, int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop,
                   const float* window, int32_t win_length, const int32_t* fb_range, const float* fb_weight, int32_t n_weights,
                   int32_t n_mels, int32_t log_base, float eps, const int32_t* tb_range, const float* tb_weight,
                   int32_t n_tweights, void* workspace, float* grad_x, void* stream);
int adk_mel_distance_grad(const float* a, const float* b, int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop,
                          const float* window, int32_t win_length, const int32_t* fb_range, const float* fb_weight,
                          int32_t n_weights, int32_t n_mels, int32_t log_base, float eps, const int32_t* tb_range,
                          const float* tb_weight, int32_t n_tweights, double scale, const float* upstream, void* workspace,
                          float* grad_a, void* stream);

/*
 * HiFi-GAN discriminator forward and its adversarial / feature-matching loss sums (models/vocoder/modules/discriminator.py:27-449,
 * losses/adversarial_loss.py, losses/feat_match_loss.py), exact f32 (the GEMM runs on the f32-input MFMA: a k-ordered fmaf chain).
 * adk_disc_conv: a non-causal, zero-padded, strided, grouped conv along H with bias and optional LeakyReLU:
 *   x [n_items][c_in][h_in][period]  ->  y [n_items][c_out][h_out][period],  h_out = (h_in + 2 pad - kernel) / stride + 1
 *   y[i][o][h'][j] = act(bias[o] + sum_{ci < c_in/groups, t < kernel} W[o][ci][t] x[i][g c_in/groups + ci][h' stride - pad + t][j])
 *   with g = o / (c_out/groups), x outside [0, h_in) read as 0, act 0 = none, 2 = LeakyReLU(slope); bias may be NULL.
 *   impl 1 (direct): w is the reference's layout [c_out][c_in/groups][kernel]; for c_in/groups == 1 or c_out/groups == 1.
 *   impl 2 (gemm):   w is [groups][c_in/groups * kernel][c_out/groups] (the reference's weight of group g, transposed).
 *   period = 1 is a Conv1d over (n_items, c_in, h_in); period = p is a (kernel, 1) Conv2d over (n_items, c_in, h_in, p).
 * adk_disc_prep: op 0 (reflect): y [rows][n_in + a] = x row, continued by reflection at its right end (F.pad 'reflect',
 *   0 <= a < n_in).  op 1 (avgpool): AvgPool1d(kernel a, stride b, padding c, count_include_pad=True):
 *   y [rows][(n_in + 2c - a) / b + 1], y[i] = (sum_{q < a} x[i b - c + q], zero outside) / a; 2c <= a.
 * adk_disc_loss FOLDS the sum over n elements of a term (f32) into a caller-owned f64 accumulator on the device:
 *   kind 0: (a-1)^2   1: a^2   2: |a - b|   3: a   4: min(a - 1, 0)   5: min(-a - 1, 0)
 *   sum [1] double += the sum;  count [1] int64 += n;  loss [1] f32 (or NULL) = sum / count after the fold (NaN while count == 0).
 * workspace: adk_disc_loss_workspace_bytes(n) bytes, 8-byte aligned, any contents (NULL when that size is 0).  Per-workgroup
 * f64 slabs and a fixed-order finalize launch: bitwise reproducible.  Calls on one accumulator must be ordered (one stream).
 * Every argument is checked before any HIP call (ADK_ERR_ARG).  No allocation, no synchronisation.
 */
int adk_disc_conv(const float* x, const float* w, const float* bias, float* y, int32_t n_items, int32_t c_in, int32_t h_in,
                  int32_t period, int32_t c_out, int32_t groups, int32_t kernel, int32_t stride, int32_t pad, int32_t act,
                  float slope, int32_t impl, void* stream);
int adk_disc_prep(const float* x, float* y, int32_t rows, int32_t n_in, int32_t op, int32_t a, int32_t b, int32_t c, void* stream);
int64_t adk_disc_loss_workspace_bytes(int64_t n);
int adk_disc_loss(const float* a, const float* b, int64_t n, int32_t kind, double* sum, int64_t* count, void* workspace,
                  float* loss, void* stream);

/*
 * HiFi-GAN discriminator backward to its input (the weights are constants), exact f32.  Every output element is written exactly
 * once, by one thread or one accumulator, with no atomics: bitwise reproducible.
 * adk_disc_conv_grad: the backward-data of adk_disc_conv with the same layer arguments:
 *   dy, y [n_items][c_out][h_out][period]  ->  dx [n_items][c_in][h_in][period]
 *   dx[i][g c_in/groups + ci][h][j] = sum over o of group g and taps t with (h + pad - t) % stride == 0 and
 *     0 <= h' = (h + pad - t) / stride < h_out  of  W[o][ci][t] dy[i][o][h'][j] (act == 2 ? (y[i][o][h'][j] > 0 ? 1 : slope) : 1)
 *   y is the layer's saved output (after the activation); read, and required, only when act == 2, which needs slope >= 0.
 *   Rows of x the forward never read get zeros.
 *   impl 1 (direct): w is the reference's layout [c_out][c_in/groups][kernel].
 *   impl 2 (gemm):   w is [groups][phase r < stride][(o, tt)][c_in/groups]: for each group and each r the taps t = r + tt stride
 *                    of every output channel o of the group, (o, tt) at o * taps(r) + tt; a K loop runs over one phase only.
 * adk_disc_prep_grad: the backward of adk_disc_prep with the same (n_in, op, a, b, c); dy has the forward's output length:
 *   op 0: dx[i] = dy[i] + dy[2 (n_in - 1) - i] where that index is in [n_in, n_in + a);
 *   op 1: dx[t] = (sum of dy[i] over the windows i b - c <= t < i b - c + a) / a.
 * adk_disc_loss_grad: grad[i] = c * d/da term(a[i], b[i]) for the kinds of adk_disc_loss:
 *   0: 2 (a - 1)   1: 2 a   2: sign(a - b), sign(0) = 0   3: 1   4: a < 1 ? 1 : 0   5: a > -1 ? -1 : 0
 *   c = (float)(coef * upstream[0]); upstream [1] f32 is read on the device.
 * Every argument is checked before any HIP call (ADK_ERR_ARG).  No allocation, no synchronisation.
 */
int adk_disc_conv_grad(const float* dy, const float* y, const float* w, float* dx, int32_t n_items, int32_t c_in, int32_t h_in,
                       int32_t period, int32_t c_out, int32_t groups, int32_t kernel, int32_t stride, int32_t pad, int32_t act,
                       float slope, int32_t impl, void* stream);
int adk_disc_prep_grad(const float* dy, float* dx, int32_t rows, int32_t n_in, int32_t op, int32_t a, int32_t b, int32_t c,
                       void* stream);
int adk_disc_loss_grad(const float* a, const float* b, int64_t n, int32_t kind, double coef, const float* upstream, float* grad,
                       void* stream);

/*
 * HiFi-GAN discriminator's own update (trainer/trainerGAN.py:256-294): the weight and bias gradient of the layer adk_disc_conv
 * computes, with the same layer arguments.  Exact f32, no atomics, every element of dw and db written once, every split of a sum
 * a function of the shape alone: bitwise reproducible.
 * adk_disc_conv_wgrad: given dy, y [n_items][c_out][h_out][period] (y the layer's saved output, after the activation) and the
 *   layer's input x [n_items][c_in][h_in][period], with g = o / (c_out/groups) and ci < c_in/groups:
 *   dz[i][o][h'][j] = dy[i][o][h'][j] (act == 2 ? (y[i][o][h'][j] > 0 ? 1 : slope) : 1)       adk_disc_conv_grad's mask, also at y == 0
 *   dw[o][ci][t]    = sum_{i,h',j} dz[i][o][h'][j] x[i][g c_in/groups + ci][h' stride - pad + t][j]   (x outside [0, h_in) is 0)
 *   db[o]           = sum_{i,h',j} dz[i][o][h'][j]                                              db [c_out] or NULL
 *   dw is [c_out][c_in/groups][kernel], the reference's layout (the period discriminator's Conv2d weight without its trailing 1).
 *   y is read, and required, only when act == 2, which needs slope >= 0.  One GEMM per group (M = c_out/groups,
 *   N = c_in/groups kernel + 1) whose reduction (i, h', j) is cut into S slices of whole 32-term steps; every (group, tile, slice)
 *   writes an f32 partial into `workspace` [slice][c_out][c_in/groups kernel + 1], and adk_conv_wgrad's fold adds a weight's S
 *   partials in ascending order in f64 and rounds once.  The mask is applied while dy is staged: no elementwise pass.  dw and db
 *   are fully written (zeros for n_items == 0, which reads nothing); with db NULL the GEMM's last column is not computed.
 *   workspace: adk_disc_conv_wgrad_plan's bytes, 4-byte aligned, any contents.
 * adk_disc_conv_wgrad_plan: host only, no HIP call: *workspace_bytes = 4 S c_out (c_in/groups kernel + 1) and *slices = S (either
 *   may be NULL).  adk_voc_conv_wgrad_plan's rule: tiles = groups ceil((c_out/groups) / BM) ceil((c_in/groups kernel + 1) / 128),
 *   BM = 128 / 64 / 32 from c_out/groups >= 128 / >= 64 / below, and n = ceil(n_items h_out period / 32) steps.
 * Every argument is checked before any HIP call (ADK_ERR_ARG): adk_disc_conv's conditions on a layer, a reduction length below
 * 2^31 - 32, c_out (c_in/groups kernel + 1) and the x offsets of an item below 2^31, groups S <= 65535.  No allocation, no
 * synchronisation.
 */
int adk_disc_conv_wgrad_plan(int32_t n_items, int32_t c_in, int32_t h_in, int32_t period, int32_t c_out, int32_t groups,
                             int32_t kernel, int32_t stride, int32_t pad, int64_t* workspace_bytes, int32_t* slices);
int adk_disc_conv_wgrad(const float* dy, const float* y, const float* x, float* dw, float* db, void* workspace, int32_t n_items,
                        int32_t c_in, int32_t h_in, int32_t period, int32_t c_out, int32_t groups, int32_t kernel, int32_t stride,
                        int32_t pad, int32_t act, float slope, void* stream);

/*
 * UnivNet spectral discriminator forward (models/vocoder/modules/discriminator.py:451-640), exact f32.  The period half of the
 * UnivNet discriminator is adk_disc_conv / adk_disc_prep, the loss sums are adk_disc_loss.
 * adk_spectrogram: torchaudio.functional.spectrogram(x, pad, window, n_fft, hop, win_length, power=1.0, normalized=False)
 *   followed by .transpose(-1, -2): x [n_signals][n_samples] gets `pad` zeros on both sides, then torch.stft's defaults
 *   (center=True with reflect padding of n_fft/2, the window zero-padded to n_fft centred, one-sided), then |X| with no eps
 *   clamp.  out [n_signals][frames][n_fft/2 + 1], frames = adk_spectrogram_frames(n_samples, pad, hop) =
 *   1 + (n_samples + 2 pad) / hop.  Both paddings and the window are applied while loading; there is no padded copy.  The FFT
 *   is adk_logmel's (one frame per wave, f64 twiddles rounded to f32).  Limits: n_fft a power of two in [256, 4096],
 *   0 < win_length <= n_fft, hop > 0, pad >= 0, n_samples + 2 pad > n_fft/2 (the reflect padding; torch raises too).
 * adk_conv2d: x [n_items][c_in][h_in][w_in] -> y [n_items][c_out][h_out][w_out], kernel (kh, kw), stride (sh, sw), zero padding
 *   (ph, pw), groups = 1, bias [c_out] (may be NULL), act 0 (none) or 2 (LeakyReLU(slope));
 *   h_out = (h_in + 2 ph - kh) / sh + 1, w_out likewise (ADK_ERR_SHAPE when the kernel is larger than the padded input).
 *   impl 1 (direct): w is the reference's [c_out][c_in][kh][kw]; for c_in = 1 or c_out = 1.
 *   impl 2 (gemm):   w is [c_in * kh * kw][c_out] (the reference's weight transposed), c_in * kh * kw <= 4096; an implicit
 *                    GEMM on the f32-input MFMA.  Both sum in the order kk = (ci*kh + th)*kw + tw, one f32 fmaf chain.
 * Every argument is checked before any HIP call (ADK_ERR_ARG / ADK_ERR_SHAPE).  No allocation, no synchronisation; results are
 * bitwise reproducible.
 */
int64_t adk_spectrogram_frames(int32_t n_samples, int32_t pad, int32_t hop);
int adk_spectrogram(const float* x, int32_t n_signals, int32_t n_samples, int32_t pad, int32_t n_fft, int32_t hop,
                    const float* window, int32_t win_length, float* out, void* stream);
int adk_conv2d(const float* x, const float* w, const float* bias, float* y, int32_t n_items, int32_t c_in, int32_t h_in,
               int32_t w_in, int32_t c_out, int32_t kh, int32_t kw, int32_t sh, int32_t sw, int32_t ph, int32_t pw, int32_t act,
               float slope, int32_t impl, void* stream);

/*
 * UnivNet spectral discriminator backward to its input (the weights are constants), exact f32.  Every output element is written
 * exactly once, by one thread or one accumulator, with no atomics: bitwise reproducible.  The period half's backward is
 * adk_disc_conv_grad / adk_disc_prep_grad, the losses' is adk_disc_loss_grad.
 * adk_conv2d_grad: the backward-data of adk_conv2d with the same layer arguments:
 *   dy, y [n_items][c_out][h_out][w_out]  ->  dx [n_items][c_in][h_in][w_in]
 *   dx[i][ci][h][w] = sum over o and taps (th, tw) with (h + ph - th) % sh == 0, (w + pw - tw) % sw == 0,
 *     0 <= h' = (h + ph - th) / sh < h_out, 0 <= w' = (w + pw - tw) / sw < w_out
 *     of  W[o][ci][th][tw] dy[i][o][h'][w'] (act == 2 ? (y[i][o][h'][w'] > 0 ? 1 : slope) : 1)
 *   y is the layer's saved output (after the activation); read, and required, only when act == 2, which needs slope >= 0.
 *   Rows and columns of x the forward never read get zeros.
 *   impl 1 (direct): w is the reference's [c_out][c_in][kh][kw]; any layer shape, meant for c_in = 1 or c_out = 1.
 *   impl 2 (gemm):   w is [phase (rh, rw), rh major][(o, tth, ttw)][c_in]: for each phase rh < sh, rw < sw the taps
 *                    th = rh + tth sh, tw = rw + ttw sw of every output channel o, (o, tth, ttw) at
 *                    (o * taps(rh) + tth) * taps(rw) + ttw; a K loop runs over one phase only.  c_out * kh * kw <= 4096.
 * adk_spectrogram_grad: the vector-Jacobian product of adk_spectrogram with respect to x.  The arguments shared with
 *   adk_spectrogram mean the same and have the same limits; g [n_signals][frames][n_fft/2 + 1] f32 is the gradient of its out,
 *   grad_x [n_signals][n_samples] f32 = sum over out of g d out / d x, as torch's autograd defines it: a bin with |X| == 0
 *   passes no gradient (abs backward, sgn(0) = 0) -- every bin of a frame that lies in the zero padding is one.
 *   Each frame's forward is recomputed; its windowed gradient goes to workspace [n_signals][frames][n_fft] f32 =
 *   adk_spectrogram_grad_workspace_bytes(n_signals, n_samples, pad, n_fft, hop) bytes, 4-byte aligned, any contents; a second
 *   launch gathers every sample's contributions through both paddings in ascending frame order.  grad_x is fully written (a
 *   sample no frame reaches gets 0).  n_signals == 0 is a no-op.
 * Every argument is checked before any HIP call (ADK_ERR_ARG / ADK_ERR_SHAPE).  No allocation, no synchronisation.
 */
int adk_conv2d_grad(const float* dy, const float* y, const float* w, float* dx, int32_t n_items, int32_t c_in, int32_t h_in,
                    int32_t w_in, int32_t c_out, int32_t kh, int32_t kw, int32_t sh, int32_t sw, int32_t ph, int32_t pw, int32_t act,
                    float slope, int32_t impl, void* stream);
int64_t adk_spectrogram_grad_workspace_bytes(int32_t n_signals, int32_t n_samples, int32_t pad, int32_t n_fft, int32_t hop);
int adk_spectrogram_grad(const float* x, const float* g, int32_t n_signals, int32_t n_samples, int32_t pad, int32_t n_fft,
                         int32_t hop, const float* window, int32_t win_length, void* workspace, float* grad_x, void* stream);

/*
 * The symmetric decoder as a frozen, differentiable function of its input (models/autoencoder/modules/decoder.py:25-138 in
 * 'causal' mode): a non-streaming forward on [n_items][c][t] tensors, the reference's layout, that writes every layer's output,
 * and the backward to the input with the weights held constant.  Exact f32 (the f32-input MFMA's k-ordered fmaf chain); every
 * output element is written exactly once, with no atomics: bitwise reproducible.
 * a is the INPUT activation: act 0 = none, 1 = ELU(alpha), a(x) = x > 0 ? x : alpha expm1(x) with the inference kernels' expm1
 * (bitwise their ELU for alpha = 1); a'(x) = x > 0 ? 1 : alpha (expm1(x) + 1).
 * adk_dec_conv: CausalConv1d.forward (layers/conv_layer.py:146-149), one group, optionally fused with a skip connection:
 *   x [n_items][c_in][t] -> y [n_items][c_out][t]
 *   y[b][o][u] = bias[o] + sum_{ci, j < kernel} W[o][ci][j] a(x[b][ci][u - (kernel-1-j) dilation]) + res[b][o][u]
 *   terms with a negative index are zero; bias [c_out] and res (of y's shape) may be NULL.
 *   impl 1 (direct): w is the reference's [c_out][c_in][kernel]; one thread per output, meant for c_out = 1 or 2.
 *   impl 2 (gemm):   w is [c_in * kernel][c_out] (the reference's weight transposed).  Both sum in the order kk = ci kernel + j.
 * adk_dec_conv_grad: its backward to x, given dy of y's shape:
 *   dx[b][ci][u] = a'(x[b][ci][u]) sum_{o, j} W[o][ci][j] dy[b][o][u + (kernel-1-j) dilation] + dres[b][ci][u]
 *   terms with an index >= t are zero; x (the forward's input) is read, and required, only when act == 1; dres (of x's shape:
 *   the gradient that reaches x through a skip connection) may be NULL.  w is [(o, j) at o kernel + j][c_in].
 * adk_dec_convtr: CausalConvTranspose1d.forward (layers/conv_layer.py:189-192) for kernel == 2 stride, the only form the
 *   reference builds: replicate padding by one frame, ConvTranspose1d, crop of one stride at both ends:
 *   x [n_items][c_in][t] -> y [n_items][c_out][t stride]
 *   y[b][o][i stride + r] = bias[o] + sum_ci W[ci][o][r] a(x[b][ci][i]) + W[ci][o][stride + r] a(x[b][ci][max(i-1, 0)])
 *   w is [r < stride][(ci, tap) at 2 ci + tap][c_out], tap 0 = W[ci][o][r], tap 1 = W[ci][o][stride + r]; bias may be NULL.
 * adk_dec_convtr_grad: its backward to x, given dy of y's shape:
 *   dx[b][ci][i] = a'(x[b][ci][i]) sum_{o, q < 2 stride} W[ci][o][q] ([i stride + q < t stride] dy[b][o][i stride + q]
 *                                                                   + [i == 0 and q >= stride] dy[b][o][q - stride])
 *   (the last term is the replicate padding's share).  w is [(o, q) at o 2 stride + q][c_in]; x as in adk_dec_conv_grad.
 * adk_rvq_st_grad: the backward of Quantizer.forward in eval mode to z (layers/vq_module.py:83-84, 119-134: the residual of
 *   stage s >= 1 is a constant to autograd, so only stage 0 passes dzq and only vqloss[0] reaches z):
 *   dz[b][c][u] = dzq[b][c][u] + up_vq[0] 2 (z[b][c][u] - codebook[idx[b t + u]][c]) / (n_items t dim)
 *   z, dzq, dz [n_items][dim][t]; codebook [size][dim], stage 0's codes; idx [n_items t] int64, stage 0's emitted indices;
 *   dzq (the gradient of zq) and up_vq (the gradient of vqloss, [n_q] f32 read on the device) may be NULL (zero).  An index
 *   outside [0, size) reads code 0 and raises bit 0 of adk_debug_flags().
 * n_items == 0 is a no-op.  Every argument is checked before any HIP call (ADK_ERR_ARG).  No allocation, no synchronisation.
 */
int adk_dec_conv(const float* x, const float* w, const float* bias, const float* res, float* y, int32_t n_items, int32_t c_in,
                 int32_t t, int32_t c_out, int32_t kernel, int32_t dilation, int32_t act, float alpha, int32_t impl, void* stream);
int adk_dec_conv_grad(const float* dy, const float* x, const float* w, const float* dres, float* dx, int32_t n_items,
                      int32_t c_in, int32_t t, int32_t c_out, int32_t kernel, int32_t dilation, int32_t act, float alpha,
                      void* stream);
int adk_dec_convtr(const float* x, const float* w, const float* bias, float* y, int32_t n_items, int32_t c_in, int32_t t,
                   int32_t c_out, int32_t kernel, int32_t stride, int32_t act, float alpha, void* stream);
int adk_dec_convtr_grad(const float* dy, const float* x, const float* w, float* dx, int32_t n_items, int32_t c_in, int32_t t,
                        int32_t c_out, int32_t kernel, int32_t stride, int32_t act, float alpha, void* stream);
int adk_rvq_st_grad(const float* dzq, const float* up_vq, const float* z, const float* codebook, const int64_t* idx, float* dz,
                    int32_t n_items, int32_t dim, int32_t t, int32_t size, void* stream);

/*
 * The encoder's training half (models/autoencoder/modules/encoder.py:25-134, 'causal' mode): the strided down-sampling conv,
 * forward and backward to its input, and the gradient of a causal conv with respect to its weight and bias.  The stride-1 layers'
 * forward and backward to the input are adk_dec_conv / adk_dec_conv_grad.  Exact f32 as the adk_dec_* calls, no atomics, every
 * split of a sum a function of the shape alone: bitwise reproducible.  a, act and alpha as above.
 * With t the input length, t_out = (t - 1) / stride + 1; terms with an index outside [0, t) or [0, t_out) are zero.
 * adk_enc_down: CausalConv1d.forward (layers/conv_layer.py:146-149) for kernel == 2 stride, dilation 1, no input activation
 *   (EncoderBlock.conv):  x [n_items][c_in][t] -> y [n_items][c_out][t_out]
 *   y[b][o][u] = bias[o] + sum_{ci, j < kernel} W[o][ci][j] x[b][ci][u stride - (kernel-1-j)]
 *   w is [c_in * kernel][c_out] (adk_dec_conv's gemm layout); bias may be NULL.
 * adk_enc_down_grad: its backward to x, given dy of y's shape:
 *   dx[b][ci][v] = sum_o sum_{j : (v + kernel-1-j) % stride == 0} W[o][ci][j] dy[b][o][(v + kernel-1-j) / stride]
 *   One GEMM per phase r = v % stride, whose two taps are j0 = (r + stride - 1) % stride (reading u0 = v / stride + (r ? 2 : 1))
 *   and j0 + stride (reading u0 - 1).  w is [r < stride][(o, tap) at 2 o + tap][c_in], tap 0 = W[o][ci][j0], tap 1 =
 *   W[o][ci][j0 + stride].  dx is fully written.
 * adk_conv_wgrad: the weight and bias gradient of a causal conv of any kernel, dilation and stride, given dy [n_items][c_out][t_out]
 *   and the conv's input x [n_items][c_in][t], which is read through a:
 *   dw[o][ci][j] = sum_{b,u} dy[b][o][u] a(x[b][ci][u stride - (kernel-1-j) dilation])     dw [c_out][c_in][kernel], the reference's
 *   db[o]        = sum_{b,u} dy[b][o][u]                                                   db [c_out] or NULL
 *   A GEMM whose reduction (b, u) is cut into S slices of whole 32-term steps; every (tile, slice) writes an f32 partial into
 *   `workspace`, and a second launch adds a weight's S partials in ascending order in f64 and rounds once.  dw and db are fully
 *   written (zeros for n_items == 0); with db NULL the GEMM's last column is not computed.  workspace: adk_conv_wgrad_plan's
 *   bytes, 4-byte aligned, any contents.
 * adk_conv_wgrad_plan: host only, no HIP call: *workspace_bytes = 4 S c_out (c_in kernel + 1) and *slices = S (either may be
 *   NULL) for a shape.  S depends on the shape alone: with tiles = ceil(c_out / BM) ceil((c_in kernel + 1) / 128), BM = 128 / 64 /
 *   32 from c_out >= 128 / >= 64 / below, and n = ceil(n_items t_out / 32) steps: S0 = max(1, min(ceil(512 / tiles), n / 4)), a
 *   slice has ceil(n / S0) steps and S = ceil(n / that), at least 1.
 * n_items == 0 is a no-op of the first two calls.  Every argument is checked before any HIP call (ADK_ERR_ARG).  No allocation, no
 * synchronisation.
 */
int adk_enc_down(const float* x, const float* w, const float* bias, float* y, int32_t n_items, int32_t c_in, int32_t t,
                 int32_t c_out, int32_t kernel, int32_t stride, void* stream);
int adk_enc_down_grad(const float* dy, const float* w, float* dx, int32_t n_items, int32_t c_in, int32_t t, int32_t c_out,
                      int32_t kernel, int32_t stride, void* stream);
int adk_conv_wgrad_plan(int32_t n_items, int32_t c_in, int32_t t, int32_t c_out, int32_t kernel, int32_t dilation, int32_t stride,
                        int64_t* workspace_bytes, int32_t* slices);
int adk_conv_wgrad(const float* dy, const float* x, float* dw, float* db, void* workspace, int32_t n_items, int32_t c_in, int32_t t,
                   int32_t c_out, int32_t kernel, int32_t dilation, int32_t stride, int32_t act, float alpha, void* stream);

/*
 * The decoder's training half: the weight and bias gradient of CausalConvTranspose1d (layers/conv_layer.py:189-192) for
 * kernel == 2 stride, the layer adk_dec_convtr computes; the decoder's stride-1 convs go through adk_conv_wgrad.  Exact f32, no
 * atomics, every split of a sum a function of the shape alone: bitwise reproducible.  a, act and alpha as above.
 * adk_convtr_wgrad: given dy [n_items][c_out][t stride] and the layer's input x [n_items][c_in][t], which is read through a:
 *   dw[ci][o][q] = sum_{b,i} a(x[b][ci][i]) g(b, o, i, q),  q < 2 stride                     dw [c_in][c_out][kernel], the reference's
 *   g            = [i stride + q < t stride] dy[b][o][i stride + q] + [i == 0 and q >= stride] dy[b][o][q - stride]
 *   db[o]        = sum_{b,u} dy[b][o][u]                                                     db [c_out] or NULL
 *   One GEMM, M = c_in, N = 2 c_out stride, whose reduction (b, i) is cut into S slices of whole 32-term steps; every (tile,
 *   slice) writes an f32 partial into `workspace`, and adk_conv_wgrad's fold adds a weight's S partials in ascending order in f64
 *   and rounds once.  db, when asked for, is a sum of its own: per channel, f64 partials of fixed chunks of (b, u), added in
 *   ascending order and rounded once.  dw and db are fully written (zeros for n_items == 0).  workspace:
 *   adk_convtr_wgrad_plan's bytes, 8-byte aligned, any contents.
 * adk_convtr_wgrad_plan: host only, no HIP call: *workspace_bytes and *slices = S (either may be NULL) for a shape.  S is
 *   adk_conv_wgrad_plan's rule with tiles = ceil(c_in / BM) ceil(2 c_out stride / 128), BM = 128 / 64 / 32 from c_in >= 128 / >= 64 /
 *   below, and n = ceil(n_items t / 32) steps.  The bytes are 4 S c_in (2 c_out stride + 1), rounded up to 8, plus 8 c_out C for
 *   db's C = ceil(L / ceil(L / min(64, ceil(L / 4096)))) chunks of L = n_items t stride terms (C = 1 for L = 0).
 * Every argument is checked before any HIP call (ADK_ERR_ARG); a stride above 18 is refused as too large.  No allocation, no
 * synchronisation.
 */
int adk_convtr_wgrad_plan(int32_t n_items, int32_t c_in, int32_t t, int32_t c_out, int32_t kernel, int32_t stride,
                          int64_t* workspace_bytes, int32_t* slices);
int adk_convtr_wgrad(const float* dy, const float* x, float* dw, float* db, void* workspace, int32_t n_items, int32_t c_in, int32_t t,
                     int32_t c_out, int32_t kernel, int32_t stride, int32_t act, float alpha, void* stream);

/*
 * The HiFi-GAN vocoder's training layers (models/vocoder/HiFiGAN.py:28-161, modules/multi_fusion.py, modules/residual_block.py):
 * the seven calls above with two extensions, on the same kernels (the adk_dec_* / adk_conv_wgrad / adk_convtr_wgrad calls are
 * these with groups = 1 and act <= 1, and their results are what they were).  Exact f32, no atomics, every output element written
 * once, every split of a sum a function of the shape alone: bitwise reproducible.
 * act: 0 = none, 1 = ELU(alpha) as above, 2 = LeakyReLU with slope alpha: a(x) = x > 0 ? x : alpha x, a'(x) = x > 0 ? 1 : alpha
 *   (the derivative at 0 is the slope, as torch's is).  x is read, and required, by the two _grad calls whenever act != 0.
 * groups = G >= 1 dividing c_in and c_out (the stride-1 calls): group g maps input channels [g c_in/G, (g+1) c_in/G) to output
 *   channels [g c_out/G, (g+1) c_out/G); with g = o / (c_out/G) and ci over c_in/G:
 *   adk_voc_conv:        y[b][o][u] = bias[o] + sum_{ci, j} W[o][ci][j] a(x[b][g c_in/G + ci][u - (kernel-1-j) dilation]) + res[b][o][u]
 *                        impl 2 (gemm): w is [G][(ci, j) at ci kernel + j][c_out/G].  impl 1 (direct): G == 1 only, meant for c_out <= 2.
 *   adk_voc_conv_grad:   dx[b][g c_in/G + ci][u] = a'(x[..]) sum_{o in g, j} W[o][ci][j] dy[b][o][u + (kernel-1-j) dilation] + dres[..]
 *                        w is [G][(o, j) at (o - g c_out/G) kernel + j][c_in/G].
 *   adk_voc_conv_wgrad:  dw[o][ci][j] = sum_{b,u} dy[b][o][u] a(x[b][g c_in/G + ci][u - (kernel-1-j) dilation]), db[o] = sum_{b,u} dy[b][o][u]
 *                        dw [c_out][c_in/G][kernel], the reference's layout; stride 1.  workspace: adk_voc_conv_wgrad_plan's bytes,
 *                        laid out [slice][c_out][c_in/G kernel + 1], so one fold serves all groups.
 *   adk_voc_conv_wgrad_plan: host only.  adk_conv_wgrad_plan's rule with tiles = G ceil((c_out/G) / BM) ceil((c_in/G kernel + 1) / 128),
 *                        BM = 128 / 64 / 32 from c_out/G >= 128 / >= 64 / below; *workspace_bytes = 4 S c_out (c_in/G kernel + 1).
 * adk_voc_convtr, adk_voc_convtr_grad, adk_voc_convtr_wgrad: adk_dec_convtr, adk_dec_convtr_grad and adk_convtr_wgrad (one group,
 *   kernel == 2 stride, the same packings; the plan is adk_convtr_wgrad_plan's) with act 0, 1 or 2.
 * n_items == 0 is a no-op of the forward and _grad calls and writes zeros for the weight gradients.  Every argument is checked
 * before any HIP call (ADK_ERR_ARG).  No allocation, no synchronisation.
 */
int adk_voc_conv(const float* x, const float* w, const float* bias, const float* res, float* y, int32_t n_items, int32_t c_in,
                 int32_t t, int32_t c_out, int32_t kernel, int32_t dilation, int32_t groups, int32_t act, float alpha, int32_t impl,
                 void* stream);
int adk_voc_conv_grad(const float* dy, const float* x, const float* w, const float* dres, float* dx, int32_t n_items,
                      int32_t c_in, int32_t t, int32_t c_out, int32_t kernel, int32_t dilation, int32_t groups, int32_t act,
                      float alpha, void* stream);
int adk_voc_convtr(const float* x, const float* w, const float* bias, float* y, int32_t n_items, int32_t c_in, int32_t t,
                   int32_t c_out, int32_t kernel, int32_t stride, int32_t act, float alpha, void* stream);
int adk_voc_convtr_grad(const float* dy, const float* x, const float* w, float* dx, int32_t n_items, int32_t c_in, int32_t t,
                        int32_t c_out, int32_t kernel, int32_t stride, int32_t act, float alpha, void* stream);
int adk_voc_conv_wgrad_plan(int32_t n_items, int32_t c_in, int32_t t, int32_t c_out, int32_t kernel, int32_t dilation,
                            int32_t groups, int64_t* workspace_bytes, int32_t* slices);
int adk_voc_conv_wgrad(const float* dy, const float* x, float* dw, float* db, void* workspace, int32_t n_items, int32_t c_in,
                       int32_t t, int32_t c_out, int32_t kernel, int32_t dilation, int32_t groups, int32_t act, float alpha,
                       void* stream);
int adk_voc_convtr_wgrad(const float* dy, const float* x, float* dw, float* db, void* workspace, int32_t n_items, int32_t c_in,
                         int32_t t, int32_t c_out, int32_t kernel, int32_t stride, int32_t act, float alpha, void* stream);

/*
 * Multi-resolution STFT loss and waveform-shape loss, one resolution / one window length per call (losses/stft_loss.py:19-170,
 * losses/waveform_loss.py:15-75).  The STFT is adk_logmel's: torch.stft's defaults, the window [win_length] centred in n_fft,
 * 1 + n_samples/hop frames, n_fft/2 + 1 bins, mag = sqrt(max(re^2 + im^2, eps)) (a NaN stays NaN).
 * adk_stft_mag writes out [n_signals][frames][n_fft/2 + 1] f32 (the layout stft() returns in the reference).
 * adk_stft_distance (x predicted, y ground truth, both [n_signals][n_samples]) FOLDS into a caller-owned accumulator on the
 * device (zero it to start; nothing is cleared here), never writing a magnitude:
 *   sums [3] double += { sum d^2 with d = y_mag - x_mag in f32,  sum y_mag^2,  sum |log y_mag - log x_mag| (correctly rounded f32 logs, f32 difference) }
 *   count [1] int64 += n_signals * frames * (n_fft/2 + 1)
 * and, from the totals after this call's fold, writes sc [1] f32 = sqrt(sums[0]) / sqrt(sums[1]) and mag [1] f32 = sums[2] / count
 * (each may be NULL; NaN while count == 0).  adk_mag_distance folds the same three sums over two given magnitude tensors of n
 * elements (SpectralConvergenceLoss / LogSTFTMagnitudeLoss take magnitudes), count += n.
 * adk_shape_distance: with windows = n_samples / winlen (the tail is dropped), a = max |y_hat| and b = max |y| over each window (a
 * NaN in the window gives NaN, as MaxPool1d):  sum [1] double += sum |a - b| (f32 difference);  count [1] int64 += n_signals *
 * windows;  loss [1] f32 (or NULL) = sum / count (NaN while count == 0).  One lane owns a window when winlen < 64, else the 64
 * lanes of a wave share it.
 * n_signals == 0 (n == 0) folds nothing.  workspace: the matching *_workspace_bytes bytes, 8-byte aligned, any contents (NULL when
 * that size is 0).  Per-workgroup f64 partials (at most 2048 workgroups, a function of the shape only) and a fixed-order
 * finalize launch: bitwise reproducible.  Calls on one accumulator must be ordered (one stream).  Limits: n_fft a power of two
 * in [256, 4096], 0 < win_length <= n_fft, hop > 0, n_samples > n_fft/2; winlen > 0, n_samples >= winlen.  Every argument is
 * checked before any HIP call (ADK_ERR_ARG).  No allocation, no synchronisation.
 */
int64_t adk_stft_workspace_bytes(int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop);
int adk_stft_mag(const float* x, int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop, const float* window,
                 int32_t win_length, float eps, float* out, void* stream);
int adk_stft_distance(const float* x, const float* y, int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop,
                      const float* window, int32_t win_length, float eps, double* sums, int64_t* count, void* workspace,
                      float* sc, float* mag, void* stream);
int64_t adk_mag_distance_workspace_bytes(int64_t n);
int adk_mag_distance(const float* x_mag, const float* y_mag, int64_t n, double* sums, int64_t* count, void* workspace, float* sc,
                     float* mag, void* stream);
int64_t adk_shape_workspace_bytes(int32_t n_signals, int32_t n_samples, int32_t winlen);
int adk_shape_distance(const float* y_hat, const float* y, int32_t n_signals, int32_t n_samples, int32_t winlen, double* sum,
                       int64_t* count, void* workspace, float* loss, void* stream);

/*
 * STFT loss and waveform-shape loss, backward (the adk_grad_* entry points, each named after the forward entry point it
 * differentiates): the vector-Jacobian products of the operations above with respect to the predicted
 * signal (x, y_hat) only, as torch's autograd defines them for losses/stft_loss.py and losses/waveform_loss.py (clamp passes the
 * gradient where its input >= eps; MaxPool1d passes it to the first maximum of a window).  Shared arguments mean the same.
 * adk_grad_stft_mag: g [n_signals][frames][n_fft/2 + 1] f32 is the gradient of adk_stft_mag's out; grad_x [n_signals][n_samples]
 * f32 = sum over out of g d out / d x.  adk_grad_stft_distance: grad_x = the gradient with respect to x of
 *   scale_sc up_sc[0] sqrt(S0) / sqrt(S1)  +  scale_mag up_mag[0] S2
 * with (S0, S1, S2) the three sums of adk_stft_distance over (x, y).  Per magnitude bin that is the product above with
 *   g = c_sc (x_mag - y_mag) - c_mag sgn / x_mag,   c_sc = (float)(scale_sc up_sc[0] / sqrt(S0 S1)), 0 where S0 == 0,
 *   c_mag = (float)(scale_mag up_mag[0]),   sgn = sign of the forward's own f32 term log y_mag - log x_mag (sign(0) = 0),
 * S0 = sums[0] and S1 = sums[1] being read on the device from the accumulator adk_stft_distance folded (x, y) into (3 doubles,
 * 8-byte aligned), up_sc / up_mag device pointers to one f32 each: nothing is read back to the host.  For the mean over R
 * resolutions, scale_sc = 1 / R and scale_mag = 1 / (R count).  Each frame's forward is recomputed (no spectra are kept); its
 * windowed gradient goes to workspace [n_signals][frames][n_fft] f32 = adk_grad_stft_workspace_bytes(...) bytes, 4-byte aligned,
 * any contents; a second launch gathers every sample's contributions through the reflect padding in ascending frame order.
 * adk_grad_shape_distance: grad [n_signals][n_samples] = the gradient with respect to y_hat of c sum |a - b|, c = (float)(scale *
 * upstream[0]): sign(a - b) sign(y_hat[i]) c at the first index i of each window's max |y_hat|, 0 at every other sample and in the
 * dropped tail.  For the mean over R window lengths, scale = 1 / (R n_signals windows).
 * No float atomics: bitwise reproducible.  grad is fully written.  n_signals == 0 is a no-op.  Same limits as the forward; every
 * argument is checked before any HIP call (ADK_ERR_ARG).  No allocation, no synchronisation.
 */
int64_t adk_grad_stft_workspace_bytes(int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop);
int adk_grad_stft_mag(const float* x, const float* g, int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop,
                     const float* window, int32_t win_length, float eps, void* workspace, float* grad_x, void* stream);
int adk_grad_stft_distance(const float* x, const float* y, int32_t n_signals, int32_t n_samples, int32_t n_fft, int32_t hop,
                           const float* window, int32_t win_length, float eps, const double* sums, double scale_sc,
                           const float* up_sc, double scale_mag, const float* up_mag, void* workspace, float* grad_x, void* stream);
int adk_grad_shape_distance(const float* y_hat, const float* y, int32_t n_signals, int32_t n_samples, int32_t winlen, double scale,
                            const float* upstream, float* grad, void* stream);

/*
 * Bit-packed code wire format (the reference passes the int64 index tensor through a
 * queue.Queue, bin/stream.py:224,230, and never serialises it).  One frame of one stream = n_q codes of
 * `bits` bits, LSB-first: code q (= emitted index - size*q) occupies bits [q*bits, (q+1)*bits) of the
 * adk_codes_frame_bytes(n_q, bits) = ceil(n_q*bits/8) byte frame; 8 x 10 bit = 10 bytes = 12.8 kbps at
 * 160 frames/s.  idx is [n_q][n_rows] int64 as emitted by adk_rvq_encode; payload is [n_rows][frame_bytes].
 * adk_codes_lookup = unpack fused into ResidualVQ.lookup (layers/vq_module.py:159-161).
 * A code >= size raises adk_debug_flags bit 2 (pack; it is packed as code 0 so that it cannot spill into the
 * neighbouring codes' bits) / bit 0 (lookup, reads code 0).
 */
int32_t adk_codes_frame_bytes(int32_t n_q, int32_t bits);
int adk_codes_pack(const int64_t* idx, uint8_t* payload, int32_t n_rows, int32_t n_q, int32_t bits, int32_t size, void* stream);
int adk_codes_unpack(const uint8_t* payload, int64_t* idx, int32_t n_rows, int32_t n_q, int32_t bits, int32_t size, void* stream);
int adk_codes_lookup(const uint8_t* payload, const float* codebook, float* zq, int32_t n_rows, int32_t n_q, int32_t bits,
                     int32_t size, int32_t dim, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pipeline level: a "program" is the fixed launch sequence of one model half (encoder+projector,
 * symmetric decoder, or HiFi-GAN vocoder) over B streams, with all rings in one caller-owned arena.
 * Replaces StreamGenerator.encode / decode (models/autoencoder/AudioDec.py:228-247,
 * models/vocoder/HiFiGAN.py:268-296) incl. the per-layer state hand-off.
 * ---------------------------------------------------------------------------------------------- */
typedef struct adk_program adk_program;

typedef struct {
    int32_t channels;    /* row length                                                               */
    int32_t hist;        /* max history any consumer needs                                           */
    int32_t rate;        /* rows per 'frame' (one hop of audio)                                      */
    int32_t external;    /* -1: lives in the arena; >= 0: index into step()'s ext[] (rows = frames*rate, cursor 0) */
    int64_t arena_off;   /* float offset of this ring in the arena (batch * rows * channels floats)  */
    int32_t extra_rows;  /* arena rings: rows beyond hist + max_frames * rate.  A ring with k * max_frames * rate extra rows still holds
                            the history of the step k steps back when the steps since have all been taken: adk_program_rewind can then be
                            applied k + 1 times in a row (the deferred guard of audiodec_amd/pipeline.py checks a step one to `depth` steps
                            late and repeats what followed it); 0 for external rings                                             */
    int32_t reserved_;   /* 0 */
} adk_ring_desc;

enum { ADK_OP_CONV = 0, ADK_OP_RING_WRITE = 1, ADK_OP_MEAN = 2,
       /* First step after create/reset only: copy the first new row of ring `in_ring` into its history rows.
          This is the replication left-pad of the NON-streaming CausalConvTranspose1d.forward
          (layers/conv_layer.py:189-192) that the offline drivers (codecTest.py / codecStatistic.py) run;
          streaming inference starts from a zero pad_buffer instead and never uses this op. */
       ADK_OP_HIST_REPLICATE = 3 };

typedef struct {
    int32_t kind;                        /* ADK_OP_*                                                  */
    int32_t in_ring, out_ring, res_ring; /* ring ids; res_ring = -1: none                             */
    int32_t in_ch_off, out_ch_off, res_ch_off;
    int32_t rate_out;                    /* output steps per frame (t_out = frames * rate_out)        */
    adk_conv_desc conv;                  /* conv.w / w_frag / bias ignored; use the offsets below     */
    int64_t w_off, wf_off, b_off;        /* float offsets into the weight blob (row-major weights, fragment-packed
                                            weights, bias); < 0: absent (at least one of w_off / wf_off)     */
    int64_t mean_off, scale_off;         /* ADK_OP_RING_WRITE: offsets of mean/scale, < 0: none       */
    int32_t ext_src;                     /* ADK_OP_RING_WRITE: index into ext[] of the source rows    */
    int32_t mean_rings[4];               /* ADK_OP_MEAN: out = (((r0 + r1) + r2) ...) / n over n_mean source rings
                                            (MultiReceptiveField: cs += block(c); c = cs / num_blocks,
                                            models/vocoder/modules/multi_fusion.py:73-79)              */
    int32_t n_mean;
    int32_t impl;                        /* ADK_IMPL_*                                                */
    int32_t fuse_next;                   /* 1: this conv's output ring is read only by the NEXT op, the 1x1 conv + residual of the same
                                            residual unit (residual_unit.py:78-81): the runner may launch both as one kernel
                                            (split-f16 rows-in-LDS kernel; the intermediate then never goes to memory) */
    int32_t chain;                       /* n >= 2: ops [this, this + n) are a residual chain -- units of (conv A; conv B + residual of A's
                                            input), each op reading the ring its predecessor writes, every intermediate ring read by nobody
                                            else (HiFiGANResidualBlock.inference, residual_block.py:99-105; the three CausalResidualUnits of
                                            an encoder / decoder block, encoder.py:76-81, decoder.py:73-78).  The runner may launch all n as
                                            ONE kernel (csrc/conv_rb16.hip: activations resident in LDS; an intermediate ring then receives
                                            only the rows later calls need as history).  0 / 1: no chain starts here */
    int32_t in_shadow, out_shadow;       /* 1 + id of the SHADOW ring of in_ring / out_ring, 0 = none (ADK_IMPL_SPLIT16* ops only).  A shadow
                                            ring has the geometry of its ring (channels, hist, rate, extra_rows; channels % 8 == 0) and holds, per
                                            8-channel group of a row (32 bytes, where the ring holds 8 floats), [8 x f16 hi][8 x f16 lo] of act(x):
                                            the split-f16 operand form the readers would otherwise recompute for every element they stage, once per
                                            tap and per 64-row tile of outputs.  out_shadow: this op writes it beside its output (stream-K kernel only:
                                            give such an op impl = ADK_IMPL_SPLIT16_SK; every op that writes the ring must carry it);
                                            in_shadow: the stream-K kernel stages from it instead of converting (other kernels ignore it:
                                            the ring itself is always complete).  Results are bit-identical with and without. */
    int32_t shadow_act;                  /* ADK_ACT_* the out_shadow carries = the act_in of the ring's readers */
    float shadow_slope;
} adk_op_desc;

/* rows of ring i = hist + max_frames * rate + extra_rows (arena rings). */
int adk_program_create(const adk_op_desc* ops, int32_t n_ops, const adk_ring_desc* rings, int32_t n_rings,
                       int32_t batch, int32_t max_frames, const float* weights, int64_t weights_floats,
                       float* arena, int64_t arena_floats, adk_program** out);
void adk_program_destroy(adk_program* p);
/* one call = `frames` hops for every stream; ext[i] are the external buffers named by the descs */
int adk_program_step(adk_program* p, int32_t frames, void* const* ext, int32_t n_ext, void* stream);
/* The same with options.  ADK_STEP_REPLAY: the ADK_OP_RING_WRITE ops are skipped -- the caller's input rows of this step are still in
 * their rings (a step that is being REPEATED after adk_program_rewind: the rows it wrote then are the rows it would write now), so the
 * repeat does not depend on the caller having kept its input buffer unchanged; ext[] entries read only by those ops may be NULL. */
enum { ADK_STEP_REPLAY = 1 };
int adk_program_step_ex(adk_program* p, int32_t frames, void* const* ext, int32_t n_ext, void* stream, int32_t step_flags);
/* reset_buffer(): zero all history (AudioDec.py:250-256, HiFiGAN.py:298-305) */
int adk_program_reset(adk_program* p, void* stream);
/* The launches of a program report device-side failures to a sticky word of the PROGRAM (same bits as adk_debug_flags, which
 * also collects the words of all live programs).  adk_program_flags waits for `stream`, returns the word and clears it (one
 * atomic exchange on the device): the caller that steps a program synchronously learns whether THIS step of THIS program
 * failed, whatever other programs run on other host threads / HIP streams.  Bit 3 (an operand of a split-f16 kernel left the
 * f16 range) is recoverable: a step only READS the history rows earlier steps left in the rings and WRITES this step's rows,
 * so adk_program_rewind(p, frames) -- cursors back by the `frames` hops of the step just taken -- followed by the same step
 * on a program lowered with the exact-f32 kernels over the same arena layout (copy the arena and the cursors across) repeats
 * it exactly; audiodec_amd/stream_generator.py does that automatically for synchronous callers ("guard"). */
int adk_program_flags(adk_program* p, void* stream, int32_t* out);
int adk_program_rewind(adk_program* p, int32_t frames);
/* The DEFERRED form of adk_program_flags, for callers that keep several steps in flight (audiodec_amd/pipeline.py, lazy_guard.py).
 * adk_program_flags_post records an event behind the launches of the step(s) just issued on `stream`; nothing waits, nothing is launched
 * (ABI 14: a program's flag word is pinned host memory its kernels report into directly; ABI 13 launched a 1-thread kernel per post).  *ticket
 * names the post (tickets count up from 0; the events of the last ADK_POST_SLOTS posts are kept).
 * adk_program_flags_poll(ticket, block): once the event has completed (block != 0: wait for it) *done = 1 and *flags = the program's word,
 * read AND cleared; else *done = 0.  ADK_ERR_STATE for a ticket that was never issued or whose slot has been reused.  With several steps of
 * one program in flight a word may already hold what a LATER step reported: a failure is attributed to the polled step or an earlier
 * one, never to a later one -- a caller that repairs by rewinding from the step a poll blames (and everything after it) is exact. */
enum { ADK_POST_SLOTS = 32 };
int adk_program_flags_post(adk_program* p, void* stream, int64_t* ticket);
int adk_program_flags_poll(adk_program* p, int64_t ticket, int32_t block, int32_t* done, int32_t* flags);
/* "Fresh" = no step since create / reset: the one state bit of a program besides its arena and cursors (the offline lowering's
 * ADK_OP_HIST_REPLICATE -- the replication pad of CausalConvTranspose1d.forward, layers/conv_layer.py:189-192 -- runs on a fresh
 * step only).  adk_program_rewind restores the value from before the rewound step -- also when it is applied several times in a row
 * (the program counts its steps since the last reset, rewinds subtracted); get / set carry the bit over to a program that takes this
 * one's place (the exact-f32 twin of the guard, also for offline programs): set(0) marks "not fresh" for good, set(1) restarts the count. */
int adk_program_get_fresh(const adk_program* p);
int adk_program_set_fresh(adk_program* p, int32_t fresh);
/* How many persistent workgroups the stream-K conv launches of this program use (multiple of 8; 0 = default = the whole
 * chip, 2 per CU).  A caller that runs several programs CONCURRENTLY on different HIP streams (software pipeline over
 * batches, bench.py) gives each a share: at 3 concurrent programs 256 measured best (210 k vs 189 k frames/s). */
int adk_program_set_workgroups(adk_program* p, int32_t workgroups);
/* Replay the steady state as HIP graphs (hipStreamBeginCapture / hipGraphLaunch): the ops between the first and the last
 * one that touch caller buffers are captured once per cursor PHASE and replayed by one hipGraphLaunch per step; the ops on
 * caller buffers (audio / codes in, waveform out) stay ordinary launches because their pointers change from call to call.
 * Ring cursors are kernel arguments, so a captured launch sequence is only valid for the cursor state it was captured in:
 * that state repeats with a short period when every ring length is a small multiple of its per-step advance
 * (max_frames * rate) -- the caller sizes the rings so by rounding `hist` up (audiodec_amd/program.py does); otherwise this
 * call fails and the program stays eager.  Only steps of exactly max_frames frames in a recognised phase, on a stream other than
 * the legacy default stream (which cannot be captured), replay; any other step (short chunk, first step after reset,
 * profiling) runs eagerly, results are identical either way.  The stream-K publish
 * flags are zeroed by a memset node at the head of each graph (their per-launch epochs are frozen by the capture). */
int adk_program_set_graph(adk_program* p, int32_t enabled);
int adk_program_graph_stats(const adk_program* p, int64_t* replays, int64_t* captures, int32_t* period);
/* ring cursors (n_rings int32), for snapshot / restore of a warmed-up state together with the arena */
int adk_program_get_cursors(const adk_program* p, int32_t* cursors, int32_t n);
int adk_program_set_cursors(adk_program* p, const int32_t* cursors, int32_t n);
/* name of the kernel op `op` runs for a `frames`-hop step (e.g. "conv_mfma<64,64>"), for profiles */
int adk_program_describe_op(adk_program* p, int32_t op, int32_t frames, char* buf, int32_t n);
/* timing aid for bench.py: per-op HIP-event durations (ms) of the LAST step when enabled; synchronises */
int adk_program_set_profiling(adk_program* p, int32_t enabled);
int adk_program_last_op_ms(adk_program* p, float* ms, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* AUDIODEC_HIP_H */
