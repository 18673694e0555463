/*
 * sfsn.h -- C ABI of libsfsn_hip.so: the MI355X (gfx950) implementation of Spiking-FullSubNet's
 * recurrent inference hot path (full-band + stacked sub-band Gated-Spiking-Neuron scans with the
 * feature prologue and deep-filter epilogue around them).
 *
 * The reference (haoxiangsnr/spiking-fullsubnet) is pure Python and has no FFI of its own; the seam this
 * ABI fills is the one SURVEY.md 8b defines: everything an `nn.Module.forward` of the reference does
 * between `stft()` and `istft()`.  Each entry point names the reference lines it replaces (paths relative
 * to the reference root):
 *     NEURON = audiozen/models/spiking_fullsubnet/efficient_spiking_neuron.py
 *     MODEL  = audiozen/models/spiking_fullsubnet/modeling_spiking_fullsubnet.py
 *     FROZEN = recipes/intel_ndns/spiking_fullsubnet_freeze_phase/model_low_freq.py
 *
 * Conventions
 *   - plain pointers, ints and floats only; no torch / HIP types in signatures (`stream` is a hipStream_t
 *     passed as void*, NULL = the null stream);
 *   - every pointer named in a launch is DEVICE memory owned by the caller; the library never allocates,
 *     frees or retains caller memory and keeps no global state: all entry points are re-entrant;
 *   - launches are asynchronous on `stream`; the return value reports argument / launch errors only;
 *   - layouts are the reference's: time-major [T][R][feat] inside a sequence model, [B][F][T] for
 *     spectra, interleaved (re, im) floats for complex64;
 *   - return codes: SFSN_OK or a negative SFSN_E* value; sfsn_strerror() names them.
 *
 * There is no CPU implementation behind this ABI and no fallback: without a gfx950 device every launch
 * returns SFSN_EHIP.
 */
#ifndef SFSN_H
#define SFSN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFSN_ABI_VERSION 21 /* bumped on every struct / signature change: a stale .so must not load */

#define SFSN_OK 0
#define SFSN_EINVAL (-1)       /* malformed argument (NULL where required, size <= 0, misaligned pointer)      */
#define SFSN_EUNSUPPORTED (-2) /* valid request the kernels do not cover (e.g. hidden size > 320)               */
#define SFSN_EHIP (-3)         /* HIP runtime error at launch (no device, invalid pointer, ...)                 */
#define SFSN_EDIVISIBLE (-4)   /* band width not divisible by the centre size: the reference's ValueError       */

#define SFSN_MAX_SEGMENTS 8    /* independent row segments (sub-band groups) per grouped launch                 */
#define SFSN_MAX_HIDDEN 320    /* largest hidden size held register-resident (baseline_m/l/xl full-band)        */
#define SFSN_MAX_GROUPS 8      /* sub-band groups per model                                                     */

int sfsn_abi_version(void);
/* First 16 hex digits of the sha256 of the sources this library was built from (include/sfsn.h and the files under csrc/): lets a binding
 * refuse a stale build whose struct layouts or entry points no longer match the header it was written against. */
const char* sfsn_source_hash(void);
const char* sfsn_strerror(int code);
/* Number of visible HIP devices (0 when there is none); never fails. */
int sfsn_device_count(void);

/* ------------------------------------------------------------------------------------------------------
 * Weight packing (HOST function, pure integer/bit work, no device needed).
 *
 * The recurrent product h.W_hh^T (NEURON:143), the layer>=2 input product S.W_ih^T (NEURON:141 with a
 * spike input) and the projection S.W_p^T (MODEL:118, FROZEN:125) all have a BINARY left operand
 * (spikes are exactly 0.0/1.0, NEURON:89).  They run on the int8 matrix cores: each fp32 weight row n is
 * split into three signed base-256 digits of a 24-bit fixed-point value with a per-row power-of-two scale,
 *     W[n][k] ~= (d2*65536 + d1*256 + d0) * dq[n],   dq[n] = 2^e[n] * 2^-23,  |W - W~| <= dq[n]/2,
 * (i.e. at most one fp32 ulp of the row's largest binade), the three int32 accumulators are exact, and
 * their recombination rounds once -- more accurate than, and independent of the summation order of, any
 * fp32 GEMM.  The digits are stored in MFMA A-fragment order for v_mfma_i32_16x16x64_i8:
 *     packed[d][nt][ks][lane][16]  with n = nt*16 + (lane & 15),  k = ks*64 + (lane >> 4)*16 + byte,
 * zero padded to NT = ceil(n_out/16) row tiles and KS = ceil(k_in/64) k-steps.
 * ---------------------------------------------------------------------------------------------------- */
size_t sfsn_w3_packed_bytes(int n_out, int k_in);               /* 3 * NT * KS * 1024 */
int sfsn_w3_padded_rows(int n_out);                            /* NT * 16 (length of dq) */
int sfsn_w3_pack(const float* w /* [n_out][k_in] host */, int n_out, int k_in, int8_t* packed /* host */,
                 float* dq /* [NT*16] host */);
/* The 16-bit-weight fast mode (BASELINE configs[2] "bf16" wording; SURVEY 0: the parity gate is the exact mode, this one reports
 * its spike agreement and output error separately): bits = 16 rounds every weight to 16 significant bits of the same per-row
 * grid and leaves the least-significant digit plane all zero; bits = 24 is sfsn_w3_pack.  Same layout, same kernels. */
int sfsn_w3_pack_bits(const float* w /* host */, int n_out, int k_in, int bits /* 24 | 16 */, int8_t* packed /* host */,
                      float* dq /* host */);
/* Inverse (tests): reconstruct W~ [n_out][k_in] from the packed digits. */
int sfsn_w3_unpack(const int8_t* packed, const float* dq, int n_out, int k_in, float* w);

/* ------------------------------------------------------------------------------------------------------
 * GSN layer scan -- replaces GSULayer.forward (NEURON:75-81: the python loop over T), GSUCell.forward
 * (NEURON:132-153) and Triangle.forward (NEURON:84-92), for several independent row segments at once
 * (the sub-band groups share H, MODEL:239-261).
 *
 * Per segment and per frame t:
 *     pre_f = zin[t][r][j] + (h . W_hh^T)[j]                               NEURON:140-145
 *     pre_g = zin[t][r][H + j] + (h . W_hh^T)[H + j]                       (unshared weights)
 *           = pre_f + (bias[H + j] - bias[j])                              (shared weights: one product serves both gates)
 *     f = sigmoid(pre_f);  c' = fma(f, c - pre_g, pre_g);  c'' = fma(c', bn_alpha[j], bn_beta[j])
 *     h' = (c'' >= 0);  carry (h', c'')                                    NEURON:146-153
 * c' is the reference's f*c + (1-f)*pre_g in the order the kernels evaluate it: the difference c - pre_g rounds before it meets f, so
 * the two forms differ by about ulp(|c| + |pre_g|) -- nothing for the gates a trained model has, 1e-5 at |pre_g| ~ 100.  The sigmoid is
 * rcp(1 + exp2(-log2(e) * pre_f)) on the hardware's exp2 / rcp.  tests/scanref.py bounds both forms; the tests cover finite inputs
 * with |pre_f|, |pre_g| <= 128 (the sigmoid's tails included: f = 0 below about -88.7, f = 1 above about 17) and no denormal results.
 * zin is the time-parallel INPUT TERM INCLUDING bias_ih, as the reference associates it ((x.W_ih^T + bias) + h.W_hh^T):
 *     shared:   zin[.][j] = (x . W_ih^T)[j] + bias[j]            (forget-gate bias; the scan adds the bias difference)
 *     unshared: zin[.][g*H + j] = (x . W_ih^T)[g*H + j] + bias[g*H + j]
 * precomputed by sfsn_input_proj_f32 / sfsn_spike_proj with their bias argument;  bn_alpha /
 * bn_beta are eval-mode BatchNorm1d folded the way ATen's CPU kernel evaluates it (alpha = gamma /
 * sqrt(var + eps), beta = fma(-mean, alpha, bias); identity = (1, 0) when bn=False).
 * The hidden state h lives in LDS as int8, the membrane c in registers, W_hh in registers as packed int8
 * digits for the whole scan; one workgroup owns 16 rows.  All segments of one launch must request the same set
 * of optional outputs (it selects the compiled kernel variant).  T is the number of frames of THIS launch: a long
 * sequence may be scanned in chunks (pointers advanced by the caller, h_state / c_state carrying the state), which is
 * how independent layers / models are pipelined over time on separate streams, and how streaming inference works.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct sfsn_scan_segment {
    const float* zin;      /* [T][R][G*H] input term incl. bias (see above), G = 1 shared / 2 unshared      */
    const int8_t* w_hh;    /* sfsn_w3_pack(W_hh [G*H][H])                                                     */
    const float* w_dq;     /* [pad16(G*H)] from sfsn_w3_pack                                                  */
    const float* bias;     /* [2H]  bias_ih                                                                   */
    const float* bn_alpha; /* [H]                                                                             */
    const float* bn_beta;  /* [H]                                                                             */
    float* h_state;        /* [R][H] in: h at t=-1 (0/1), out: h at t=T-1   (NEURON:50-62 state in/out)       */
    float* c_state;        /* [R][H] in/out membrane                                                          */
    float* spikes_f32;     /* [T][R][H] out, nullable  (the reference's all_layer_outputs entry)              */
    int8_t* spikes_i8;     /* [T][R][pad64(H)] out, REQUIRED (B operand of the next sfsn_spike_proj)         */
    float* membrane;       /* [T][R][H] out, nullable  (post-BN membrane; parity tests only; needs spikes_f32)*/
    int R;                 /* rows in this segment (> 0)                                                      */
    unsigned long long* spike_count; /* nullable, 8-byte aligned (ABI 16).  When spikes_f32 is NULL the launch ADDS the number
                            * of spikes it wrote for this segment (rows < R, neurons < H, its T frames) -- the reduction
                            * audiozen/metric.py:303-340 takes of an all_layer_outputs entry, formed inside the scan:
                            * zero it once per forward, chunked calls accumulate.  Ignored when spikes_f32 is given. */
} sfsn_scan_segment;

int sfsn_gsn_layer_scan(const sfsn_scan_segment* segs /* host array */, int n_segs, int T, int H, int shared,
                        int rows_per_wg /* 16, 8, 4, or 0 = choose so that the launch covers ~all CUs */, void* stream);

/* The same scan for weights packed with 16 bits (sfsn_w3_pack_bits(.., 16): digit plane 0 is zero): the zero plane's matrix
 * instructions are skipped (8 instead of 12 per tile and step; the sums are the same, so the results equal sfsn_gsn_layer_scan's
 * on the same packed weights).  Covers what the IO-specialised scan covers (shared gates, H <= 224, 4 or 8 rows per workgroup, no
 * membrane output); SFSN_EUNSUPPORTED otherwise -- the caller then uses sfsn_gsn_layer_scan.  BASELINE configs[2]'s 16-bit mode. */
int sfsn_gsn_layer_scan_w16(const sfsn_scan_segment* segs /* host */, int n_segs, int T, int H, int shared, int rows_per_wg, void* stream);

/* Separate gate weights that do not fit one compute unit (shared = 0, H > 256: baseline_xl's full-band model, 2 x 320 x 320 x 3 bytes):
 * sfsn_gsn_layer_scan streams all of W_hh from the L2 every step (10 us per step); here the neuron tiles of a 16-row block are split
 * over several workgroups that keep their share resident in LDS and exchange the new spikes every step through `scratch`
 * (sfsn_scan_split_scratch_bytes(R, H) bytes, 16-byte aligned, ZEROED by the caller before every call; its first word is a sticky
 * error word: non-zero = a bounded wait expired, the outputs are invalid).  Same results as sfsn_gsn_layer_scan, bit for bit.  One
 * segment; ceil(R / 16) x splits workgroups must be co-resident (<= compute units): SFSN_EUNSUPPORTED otherwise, and for shapes
 * sfsn_gsn_layer_scan serves from one compute unit.  (ABI 17) */
size_t sfsn_scan_split_scratch_bytes(int R, int H);
int sfsn_gsn_layer_scan_split(const sfsn_scan_segment* segs /* host */, int n_segs, int T, int H, int shared, void* scratch,
                              size_t scratch_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Training-mode cell steps -- replace one iteration of GSULayer.forward's loop (NEURON:78-80) around
 * GSUCell.forward (NEURON:132-153) with nn.BatchNorm1d in TRAINING mode (batch statistics of this step over all R rows, running
 * statistics updated with `momentum`, NEURON:123,149-150), and the matching step of the backward pass through Triangle.backward
 * (NEURON:94-101).  One launch per time step: the rows of a step are coupled by the normalisation.  All tensors fp32, device.
 *   z [R][G*H]: x_t . W_ih^T WITHOUT bias (G = 1 shared: one product serves both gates; 2: forget | cell);  bias [2H];
 *   w_hh [G*H][H] fp32;  h_prev [R][H] spikes (0 / 1: anything non-zero counts as 1), c_prev [R][H];  bn_w / bn_b [H] (both NULL: bn = False);  running_mean / running_var [H]
 *   nullable (not updated).  Outputs of the forward step (saved for the backward step): spikes = h_t, u = c_t (post-BN
 *   membrane), xhat (normalised, pre-affine; bn only), f (forget gate), g (pre-activation of the cell gate), invstd [H] (bn only).
 * Backward step: dh_up (gradient w.r.t. h_t from above, nullable), dh_rec (gradient w.r.t. h_t through step t+1's recurrent
 *   product, nullable), dc_next (gradient w.r.t. c_t from step t+1, nullable) -> d_gates [R][2H] (d pre_f | d pre_g), d_z [R][G*H]
 *   (shared: their sum = the gradient of the shared product; unshared: pass NULL and use d_gates), dc_prev [R][H], and
 *   d_bn_w / d_bn_b [H] ACCUMULATED (+=).  The recurrent part of dL/dh_t is either handed in (dh_rec) or formed by the step itself
 *   from the previous launch's d_z (dz_next . W_hh: no GEMM launch between the steps).
 * Rows per step beyond ~64 are spread over several workgroups per neuron tile, which exchange their partial sums through `scratch`
 * (sfsn_train_scratch_bytes(H) bytes, ZEROED by the caller before the first step of a layer call: 8-byte {value, epoch} granules)
 * and wait for each other inside the launch; `epoch` = 1, 2, ... counts the steps issued on that scratch buffer (forward and backward use their own buffers). */
size_t sfsn_train_scratch_bytes(int H);
/* SFSN_OK when BOTH step kernels take this geometry (their LDS needs differ): call once per layer before the first forward step. */
int sfsn_gsn_train_check(int R, int H, int shared);
/* The same question for the per-step launches alone (their own, smaller LDS needs; with several row blocks per neuron tile also that
 * a step launch can hold its workgroups resident: needs the device then).  training.py asks it before it falls back from the one-launch
 * layer call (sfsn_gsn_train_multi_check said SFSN_EUNSUPPORTED) to a launch per step, and for the eval-mode-BatchNorm path.  ABI 16. */
int sfsn_gsn_train_step_check(int R, int H, int shared);
int sfsn_gsn_train_step_fwd(const float* z, const float* w_hh, const float* bias, const float* h_prev, const float* c_prev,
                            const float* bn_w, const float* bn_b, float* running_mean, float* running_var, float momentum, float eps,
                            int R, int H, int shared, float* spikes, float* u, float* xhat, float* f, float* g, float* invstd,
                            void* scratch, unsigned epoch, void* stream);
int sfsn_gsn_train_step_bwd(const float* dz_next /* [R][G*H] d_z of step t+1, nullable */, const float* w_hh /* [G*H][H] */,
                            const float* dh_up, const float* dh_rec, const float* dc_next, const float* u, const float* xhat,
                            const float* f, const float* g, const float* c_prev, const float* invstd, const float* bn_w, int R, int H,
                            int shared, float* d_gates, float* d_z, float* dc_prev, float* d_bn_w, float* d_bn_b, void* scratch,
                            unsigned epoch, void* stream);

/* A whole layer call in ONE launch (ABI 14; ABI <= 13 enqueued T step launches): forward (t = 0 .. T-1) or backward (t = T-1 .. 0).
 * The workgroups stay resident for all T steps -- weight tile, carried membrane (forward) / its gradient (backward) in LDS -- and
 * exchange what a step needs from other workgroups through the L2 (csrc/sfsn_train.hip: packed spikes / d_z written through, one
 * publish counter per row block; the BatchNorm partial sums as for the step entries).  Every expression but the two products
 * (h_{t-1} . W_hh^T forward, d_z_{t+1} . W_hh backward) is the step entries', operation for operation; the products differ in
 * SUMMATION ORDER -- the step entries run one fma chain in k order, these kernels v_mfma_f32_16x16x4_f32 (k = 16 s + 4 q + e, the
 * four q of an instruction summed inside it) -- so the two families agree within rounding, not bit for bit: a membrane closer to the
 * threshold than the rounding error of u (tests/trainref.py: fwd_bound's bound on u) may spike in one and not in the other.  Both
 * lie within that fp64 bound on the same inputs (tests/test_train_edges.py); a call cut into chunks of frames (below) equals the
 * uncut call bit for bit.  Tensors as for the step entries with a leading [T]: z [T][R][G*H]; spikes, u, xhat, f, g, dh_up
 * [T][R][H]; invstd [T][H];
 * d_gates [T][R][2H]; d_z [T][R][H] (shared; NULL otherwise).  Zero initial state (MODEL:100-106).  `zero` and `dc_work` are unused
 * (kept for the ABI-13 call shape; may be NULL).  `scratch`: sfsn_train_seq_scratch_bytes(R, H) bytes, ZEROED by the caller before the
 * call, one buffer per call (forward and backward use their own); its last four 32-bit words hold the error word as before. */
size_t sfsn_train_seq_scratch_bytes(int R, int H);
/* Several layer calls of the same (T, H, gate sharing) in ONE launch per direction -- the sub-band groups of a model are independent
 * of one another, and a layer call leaves most of the chip idle: their workgroups sit side by side in one grid.  Per call the
 * tensors of sfsn_gsn_train_seq_fwd / _bwd and its own zeroed scratch buffer.  n <= 8.  All calls with BatchNorm or all without.
 * SFSN_EUNSUPPORTED when the launch could not hold every call's workgroups resident together (sfsn_gsn_train_multi_check says so
 * up front; it needs the device): issue the calls separately then.  A launch with more calls than fit at the single call's geometry
 * (~160 workgroups per call) gives ALL its calls fewer, larger row blocks, per direction, until it fits or a block's rows exceed the
 * LDS (round 5: the layers of several stacks side by side, training.GSNStackTrainFn); the BatchNorm partial sums are then merged in
 * another blocking (last-bit differences against the single call). */
typedef struct {
    const float *z, *w_hh, *bias, *bn_w, *bn_b;
    float *running_mean, *running_var;
    float momentum, eps;
    int R;
    float *spikes, *u, *xhat, *f, *g, *invstd;
    void* scratch;
    /* ABI 17: a layer call cut into CHUNKS of frames (so that layer l + 1 can work on chunk c while layer l works on chunk c + 1 in the
     * same launch: two calls of one multi launch).  h0 / c0 [R][H], both or neither: the spikes and the (post-BatchNorm) membrane of the
     * frame before this call's first -- rows `spikes[-1]` / `u[-1]` of the previous chunk's call; NULL = zero state.  The running
     * statistics continue through the calls in launch order; momentum < 0 counts from the batches tracked before THIS call. */
    const float *h0, *c0;
    int T; /* > 0: this call's own frame count (chunks of unequal length side by side); 0: the launch's T */
} SfsnTrainSeqFwd;
typedef struct {
    const float *w_hh, *dh_up, *u, *xhat, *f, *g, *invstd, *bn_w;
    int R;
    float *d_gates, *d_z, *d_bn_w, *d_bn_b;
    void* scratch;
    /* ABI 17, chunked calls (issued last chunk first): dc_in [R][H] = dL/dc carried out of the chunk BEHIND this one (its dc_out); with it
     * the tensors must continue behind this call's T frames -- d_z / d_gates frame T is that chunk's first, already written.  dc_out
     * [R][H], nullable: dL/dc carried out of this call's first frame.  has_prev: `u` has a frame before this call's first (u - R*H floats:
     * the membrane the first step's forget gate multiplied), i.e. this is not the sequence's first chunk. */
    const float* dc_in;
    float* dc_out;
    int has_prev;
    int T; /* > 0: this call's own frame count; 0: the launch's T */
} SfsnTrainSeqBwd;
int sfsn_gsn_train_multi_check(const int* R, int n, int H, int shared);
int sfsn_gsn_train_seq_fwd_multi(const SfsnTrainSeqFwd* calls, int n, int T, int H, int shared, void* stream);
int sfsn_gsn_train_seq_bwd_multi(const SfsnTrainSeqBwd* calls, int n, int T, int H, int shared, void* stream);
int sfsn_gsn_train_seq_fwd(const float* z, const float* w_hh, const float* bias, const float* bn_w, const float* bn_b,
                           float* running_mean, float* running_var, float momentum, float eps, int T, int R, int H, int shared,
                           const float* zero, float* spikes, float* u, float* xhat, float* f, float* g, float* invstd, void* scratch,
                           void* stream);
int sfsn_gsn_train_seq_bwd(const float* w_hh, const float* dh_up, const float* u, const float* xhat, const float* f, const float* g,
                           const float* invstd, const float* bn_w, int T, int R, int H, int shared, const float* zero, float* d_gates,
                           float* d_z, float* dc_work, float* d_bn_w, float* d_bn_b, void* scratch, void* stream);

/* Fused-input variant for layers >= 1 (their input is the previous layer's spikes): the input term is computed inside
 * the scan from the int8 spikes and the packed input weights, so that sfsn_spike_proj's [T][R][H] fp32 result never makes
 * its round trip through HBM.  Bit-identical to sfsn_spike_proj(bias = bias[0:H]) + sfsn_gsn_layer_scan.  Shared gate
 * weights, 128 < H <= 256, 16 rows per workgroup (the geometry for a full chip); `zin` and `membrane` of the segments are
 * ignored / must be NULL.  SFSN_EUNSUPPORTED for other shapes: the caller then uses the two-call form. */
typedef struct sfsn_fused_input {
    const int8_t* spikes_in; /* [T][R][pad64(H)] the previous layer's spikes_i8                           */
    const int8_t* w_ih;      /* sfsn_w3_pack(W_ih [H][H])                                                  */
    const float* w_ih_dq;    /* [pad16(H)]                                                                 */
} sfsn_fused_input;

int sfsn_gsn_layer_scan_fused(const sfsn_scan_segment* segs /* host */, const sfsn_fused_input* fin /* host, one per segment */,
                              int n_segs, int T, int H, void* stream);

/* Layer-0 twin: the real-valued input product inside the scan (bf16 3-way split, bit-identical to sfsn_input_proj_f32 +
 * sfsn_gsn_layer_scan).  Same restrictions as above plus: I even, I <= 64, R % 16 == 0, x 16-byte aligned.  All segments of
 * a launch see the same LDS layout only if they share I: the slot size is taken from each segment's own I. */
typedef struct sfsn_fused_x {
    const float* x;    /* [T][R][I] the layer input (sfsn_features' output) */
    const float* w_ih; /* [H][I] fp32 input weights, row-major              */
    int I;
} sfsn_fused_x;

int sfsn_gsn_layer_scan_fused_x(const sfsn_scan_segment* segs /* host */, const sfsn_fused_x* fin /* host, one per segment */,
                                int n_segs, int T, int H, void* stream);

/* Layer 0 of several groups in ONE launch at 16 rows per workgroup: the segments of a sfsn_gsn_layer_scan_fused_x call (segs_x / fin_x,
 * n_x of them; their workgroups come first) and those of a sfsn_gsn_layer_scan(.., shared, 16, ..) call (segs_z, n_z of them, each with
 * its `zin`) side by side, every workgroup running the kernel body its own entry point would have launched: bit-identical to the two
 * calls, one launch instead of two in a row.  Each list is checked as its own entry point checks it (the fused-x list first, same
 * answers in the same order).  SFSN_EUNSUPPORTED -- the caller makes the two calls -- where either list would not take its 16-row
 * kernel (H > 224, separate gate weights, a membrane output, SFSN_SCAN_V2 / SFSN_FUSED_V2 set), where the two lists differ in their
 * output set, hold more than SFSN_MAX_SEGMENTS segments together, or one of them is empty. */
int sfsn_gsn_layer_scan_l0(const sfsn_scan_segment* segs_x /* host */, const sfsn_fused_x* fin_x /* host, one per segment of segs_x */,
                           int n_x, const sfsn_scan_segment* segs_z /* host */, int n_z, int T, int H, int shared, void* stream);

/* Layer-pipelined stack scan -- replaces StackedGSU.forward (NEURON:50-62) for ALL layers of a stack in ONE launch.
 * The reference runs layer l over all T frames, then layer l+1 (NEURON:56-61); layer l+1 needs frame t of layer l only at
 * frame t, so here every layer's rows get their own workgroups (weights resident for the whole launch) and the workgroups of
 * layer l+1 trail their producers of layer l by a few frames: int8 spikes handed over through L2 with write-through stores and
 * per-workgroup progress counters.  The critical path of a stack is one chain of T steps instead of n_layers chains, and the
 * fp32 input term of layers >= 1 makes no round trip through HBM.  Bit-identical to sfsn_input_proj_f32 / sfsn_spike_proj +
 * sfsn_gsn_layer_scan per layer.
 *   segs[l * n_segs + i]: layer l of segment i, as for sfsn_gsn_layer_scan; `zin` is read for layer 0 (the input term incl.
 *       bias, written before the launch).  For H > 256 (the two matrices of a layer >= 1 do not fit one CU) `zin` of layers >= 1
 *       must point at a [T][R][H] scratch buffer: a third kind of workgroup computes the input term into it, frame by frame.
 *       `membrane` must be NULL.  R of a segment is the same in every layer.
 *   fin[l * n_segs + i]: packed input weights of layer l >= 1; spikes_in must equal segs[(l-1) * n_segs + i].spikes_i8.
 *   rows_per_wg[l]: 4, 8 or 16 (NULL: 8 everywhere).  One workgroup occupies a CU: keep the sum over all layers of
 *       ceil(R / rows_per_wg) within the device's CU count, or layers queue behind each other (correct, not pipelined).
 *   lag: frames a consumer lets its producers run ahead before it (re)starts -- amortises its polls; 16-32 is a good value.
 *   scratch: device memory, sfsn_stack_scratch_bytes(...) bytes, ZEROED by the caller once (before its first use) and private to
 *       the launches that use it, one at a time: every launch leaves its counters zeroed again (its last workgroup does it -- no
 *       memset per launch).  Word 0 is an error flag the caller may read back after a launch: non-zero = a bounded hand-off
 *       wait expired (results invalid); the library never clears it.
 * Shared gate weights only (SFSN_EUNSUPPORTED otherwise: use the per-layer calls). */
size_t sfsn_stack_scratch_bytes(int n_layers, int n_segs, int rows_total);
int sfsn_gsn_stack_scan(const sfsn_scan_segment* segs /* host [n_layers][n_segs] */, const sfsn_fused_input* fin /* host, same shape;
                        layer-0 entries ignored */, int n_layers, int n_segs, int T, int H, const int* rows_per_wg /* host [n_layers] */,
                        int lag, void* scratch, size_t scratch_bytes, void* stream);
/* The same with layer 0's real-valued input product inside the scan for the segments whose fx[i].x is given (round 4; fx NULL or
 * fx[i].x NULL: the segment's layer 0 reads `zin` as above): x [T][R][I] fp32 and W_ih [H][I] fp32 as for
 * sfsn_gsn_layer_scan_fused_x -- the bf16 3-way split of sfsn_input_proj_f32, bit-identical to that call + the scan.  Needs the
 * layout this entry point gives stacks of H <= 224 without input-term buffers (or a single layer): 8 rows per workgroup in every
 * layer, even I <= 64, R a multiple of 8, x 16-byte aligned; SFSN_EUNSUPPORTED otherwise (use `zin`). */
int sfsn_gsn_stack_scan_x(const sfsn_scan_segment* segs, const sfsn_fused_input* fin, const sfsn_fused_x* fx /* host [n_segs], nullable */,
                          int n_layers, int n_segs, int T, int H, const int* rows_per_wg, int lag, void* scratch, size_t scratch_bytes,
                          void* stream);
/* Layers 0 AND 1 of a two-layer stack in ONE launch at 16 rows per workgroup: the workgroups of a sfsn_gsn_layer_scan_l0 call (segs_x /
 * fin_x, then segs_z; either list may be empty, not both) and, behind them, those of the sfsn_gsn_layer_scan_fused call of layer 1
 * (segs1 / fin1: n_x + n_z entries in the order x then z), every workgroup running the kernel body its own entry point would have
 * launched.  A layer-1 workgroup trails the layer-0 workgroup of the same 16 rows by a few frames (write-through int8 rows, a progress
 * counter per workgroup, sc1 loads: the hand-off of sfsn_gsn_stack_scan).  Bit-identical to the two calls.
 *   fin1[i].spikes_in must be the spikes_i8 of layer-0 segment i and the row counts must agree (SFSN_EINVAL otherwise).
 *   Each list is checked as its own entry point checks it (fused-x, then the input-term list, then layer 1).
 *   SFSN_EUNSUPPORTED -- the caller makes the per-layer calls -- where one of the lists would not take its 16-row IO-wave kernel
 *   (H > 224, separate gate weights, a membrane output, SFSN_SCAN_V2 / SFSN_FUSED_V2 set), where the lists differ in their output set,
 *   or the layer holds more than SFSN_MAX_SEGMENTS segments.
 *   lag, scratch (sfsn_stack_scratch_bytes(2, n_x + n_z, rows of a layer) bytes), error word: as for sfsn_gsn_stack_scan. */
int sfsn_gsn_layer_scan_l01(const sfsn_scan_segment* segs_x /* host */, const sfsn_fused_x* fin_x /* host, one per segment of segs_x */,
                            int n_x, const sfsn_scan_segment* segs_z /* host */, int n_z, const sfsn_scan_segment* segs1 /* host */,
                            const sfsn_fused_input* fin1 /* host, one per segment of segs1 */, int T, int H, int shared, int lag,
                            void* scratch, size_t scratch_bytes, void* stream);
/* Round 6 (ABI 19): the same launch for weights packed with 16 bits (sfsn_w3_pack_bits(w, n, k, 16, ..): the least significant digit plane
 * of every recurrent / spike-input matrix is zero): the zero plane's matrix instructions are skipped in the IO-wave scan, FUSEDX3 and FUSED3
 * roles of the sub-band pair layout (8 rows per workgroup, no input-term buffers for the layers >= 1, H <= 224) -- the same sums, hence the
 * same results as sfsn_gsn_stack_scan_x on such weights.  SFSN_EUNSUPPORTED for every other layout.  BASELINE configs[2]'s 16-bit mode
 * (module.weight_bits = 16): a report mode, not the fp32 parity mode. */
int sfsn_gsn_stack_scan_x_w16(const sfsn_scan_segment* segs, const sfsn_fused_input* fin, const sfsn_fused_x* fx /* host [n_segs], nullable */,
                          int n_layers, int n_segs, int T, int H, const int* rows_per_wg, int lag, void* scratch, size_t scratch_bytes,
                          void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Time-parallel products.
 * sfsn_input_proj_f32: z[m][n] = sum_k x[m][k] * w[n][k] (+ bias[n])  (NEURON:141-142 for layer 0: real-valued x)
 *     fp32-accurate on the bf16 matrix cores: x and w are split (round to nearest) into three bf16 pieces each, the six
 *     leading piece products are exact in fp32 and carry x.w to 2^-26 |x||w| per term, accumulation in fp32
 *     (even K <= 192); v_mfma_f32_16x16x4_f32 (an exact k-ordered fmaf chain) for the other shapes.
 *     x [M][K], w [N][K] row-major fp32, z [M][ldz] (columns 0..N-1 written; ldz > N lets the two gate halves of an
 *     unshared cell land side by side).
 * sfsn_spike_proj:     y[m][n] = dq[n] * sum_k s[m][k] * Wq[n][k] (+ bias[n])
 *     s int8 0/1 [M][pad64(K)] as written by the scan; Wq/dq from sfsn_w3_pack(W [N][K]); y [M][N] fp32.
 *     Used for layer>=1 input products (bias NULL: NEURON:141) and the projection (nn.Linear MODEL:49-52,118;
 *     FROZEN:71-76,125: bias added after the product).
 * ---------------------------------------------------------------------------------------------------- */
int sfsn_input_proj_f32(const float* x, const float* w, const float* bias /* [N], nullable */, float* z, int M, int K, int N,
                        int ldz /* >= N: row stride of z */, void* stream);

/* Several products in ONE launch (ABI 16): the projections (or the layer-0 input products) of the sub-band groups of a chunk are
 * independent of one another (MODEL:118,141 per sequence model); each alone leaves compute units idle and pays a launch boundary.
 * Same results as one sfsn_spike_proj / sfsn_input_proj_f32 call per job (every workgroup runs its job's own tiling).  n <= 8; all
 * spike jobs share ceil(K / 64).  SFSN_EUNSUPPORTED when a job would not take the single entry's fast kernel (N % 4, ld % 4, M < 64,
 * an unaligned output, N > 256, odd K / K > 192 for the real-valued product): issue the calls one by one then. */
typedef struct sfsn_proj_job {
    const int8_t* s;        /* [M][pad64(K)] int8 spikes */
    const int8_t* w_packed; /* sfsn_w3_pack(W [N][K])     */
    const float* w_dq;
    const float* bias;      /* [N], nullable */
    float* y;               /* [M][ldy] */
    int M, K, N, ldy;
} sfsn_proj_job;
int sfsn_spike_proj_multi(const sfsn_proj_job* jobs /* host */, int n, void* stream);
typedef struct sfsn_inproj_job {
    const float* x;    /* [M][K] */
    const float* w;    /* [N][K] */
    const float* bias; /* [N], nullable */
    float* z;          /* [M][ldz] */
    int M, K, N, ldz;
} sfsn_inproj_job;
int sfsn_input_proj_f32_multi(const sfsn_inproj_job* jobs /* host */, int n, void* stream);
int sfsn_spike_proj(const int8_t* s, const int8_t* w_packed, const float* w_dq, const float* bias /* nullable */,
                    float* y, int M, int K, int N, int ldy /* >= N: row stride of y */, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Feature prologue -- replaces MODEL:434-440 (|X|^fdrc, drop Nyquist, band select), SubbandModel.forward's
 * two _freq_unfold calls + cat (MODEL:239-258, 265-312; FROZEN:350-431,451-474), the "b f t -> t b f"
 * transposes (MODEL:108,155) and the input normalisation: nn.LayerNorm (MODEL:27-28,111-112) or the frozen
 * model's offline_laplace_norm (FROZEN:147-169, 475, 578).
 *
 * A feature group g produces x_g [T][B*N][I], row r = b*N + k, I = (ctr + 2 nbr) + (ctr_fb + 2 nbr_fb):
 *     j <  ctr+2nbr : mag[b][reflect(lo + k*ctr - nbr + j)][t]            (reflect: f<0 -> -f, f>nf-1 -> 2(nf-1)-f)
 *     j >= ctr+2nbr : fb[t][b][reflect(lo + k*ctr_fb - nbr_fb + j') % FB]  (the tiled full-band output, MODEL:442-443)
 * with mag = |stft|^fdrc on bins 0..nf-1 (nf = F-1).  The full-band model's own input is the group
 * {lo=0, n_units=1, ctr=FB, nbr=0, ctr_fb=0}.
 * Input domain: every |stft| is 0 or lies in [2^-60, 2^60] -- the magnitude is sqrt(fma(re, re, im * im)) in fp32 without range
 * scaling (sfsn_feat_dev.h), so values outside it may lose bits to underflow or overflow of the squares.  The same domain holds for
 * sfsn_laplace_means, sfsn_gaussian_stats and the enh_mag outputs of the deep-filter entry points.
 * ---------------------------------------------------------------------------------------------------- */
#define SFSN_NORM_NONE 0
#define SFSN_NORM_LAYERNORM 1 /* (x - mean) * rstd * ln_w + ln_b over the I features, eps inside the sqrt       */
#define SFSN_NORM_LAPLACE 2   /* x / (mu[b] + 2.220446049250313e-16), mu from sfsn_laplace_means                 */
#define SFSN_NORM_GAUSSIAN 4   /* (x - mu[b]) / (sd[b] + 2.220446049250313e-16), mu / sd from sfsn_gaussian_stats; sd is passed in ln_w */
#define SFSN_NORM_CUMLAPLACE 3 /* sfsn_stream_hop only: x / (running mean of the row + eps), state carried per row -- the offline
                                  path runs sfsn_features with SFSN_NORM_NONE and then sfsn_cum_laplace_norm             */

typedef struct sfsn_feature_group {
    float* x;           /* out [T][B*n_units][I]                                                             */
    const float* ln_w;  /* [I] (LAYERNORM); GAUSSIAN: [B] the clips' standard deviations                      */
    const float* ln_b;  /* [I] (LAYERNORM)                                                                    */
    const float* mu;    /* [B] (LAPLACE, GAUSSIAN)                                                            */
    int lo, n_units, ctr, nbr, ctr_fb, nbr_fb;
    int norm;           /* SFSN_NORM_*                                                                        */
    float ln_eps;
} sfsn_feature_group;

int sfsn_features(const float* stft_ri /* [B][F][T][2] */, const float* fb_tbf /* [T][B][FB], NULL if unused */,
                  int B, int F, int T, int FB, float fdrc, const sfsn_feature_group* groups /* host */, int n_groups,
                  int t0, int nt /* frames [t0, t0+nt) are produced; tensors are indexed by absolute frame */, void* stream);
/* The same launch with a side job: extra workgroups zero `zero_bytes` bytes at `zero_ptr` (both multiples of 16) -- the zero initial
 * state of the forward's scans (MODEL:100-106) written by the first launch of the forward's chain instead of a fill launch of its own. */
int sfsn_features_z(const float* stft_ri, const float* fb_tbf, int B, int F, int T, int FB, float fdrc, const sfsn_feature_group* groups,
                    int n_groups, int t0, int nt, float* zero_ptr, size_t zero_bytes, void* stream);

/* The feature prologue AND the layer-0 input product of a chunk in ONE launch (ABI 17) -- replaces, for every job, the pair
 * sfsn_features + sfsn_input_proj_f32 (MODEL:434-440,239-258,108-112 followed by NEURON:141-142): a workgroup keeps the rows it has
 * normalised, splits them into the three bf16 pieces from registers and forms x . W_ih^T + b on the bf16 matrix cores; the rows go
 * to HBM only when `feat.x` is given (the API's all_layer_outputs[0], or a scan that forms its product itself).  A job with w = NULL
 * is sfsn_features alone for that group (feat.x required).  Bit-identical to the two calls: the rows by features_kernel's
 * expressions and wave reductions, the products by input_proj_bf3_kernel's six piece products in its order.
 * z is CHUNK-LOCAL: [nt][B * n_units][ldz], frame t0 first (x is indexed by absolute frame, as in sfsn_features).
 * SFSN_EUNSUPPORTED for what sfsn_input_proj_f32 would not run on its bf16-split kernel (odd I, I > 160 with H > 128, H > 384,
 * fewer than 64 rows, SFSN_INPROJ_F32 set) and for groups reading more than 144 bins or FB > 128: issue the two calls then. */
typedef struct sfsn_featproj_job {
    sfsn_feature_group feat; /* feat.x nullable when w is given */
    const float* w;          /* [H][I] fp32 W_ih (shared gates), NULL = rows only                                */
    const float* bias;       /* [H], nullable                                                                     */
    float* z;                /* out [nt][B*n_units][ldz]                                                          */
    int H, ldz;
} sfsn_featproj_job;
int sfsn_features_proj(const float* stft_ri, const float* fb_tbf, int B, int F, int T, int FB, float fdrc,
                       const sfsn_featproj_job* jobs /* host */, int n_jobs, int t0, int nt, float* zero_ptr /* as sfsn_features_z */,
                       size_t zero_bytes, void* stream);

/* Per-clip means for offline_laplace_norm (FROZEN:162-164: mean over all non-batch dims of the gathered,
 * un-normalised group tensor).  mu_out [n_groups][B].  Two launches: row sums of mag / fb, then the
 * weighted combination; `scratch` needs B*(F-1+FB) floats. */
int sfsn_laplace_means(const float* stft_ri, const float* fb_tbf, int B, int F, int T, int FB, float fdrc,
                       const sfsn_feature_group* groups /* host, only geometry fields are read */, int n_groups,
                       float* mu_out, float* scratch, void* stream);
/* Per-clip mean and UNBIASED standard deviation for offline_gaussian_norm (FROZEN:205-218: torch.mean / torch.std over all non-batch
 * dims of the gathered, un-normalised group tensor).  mu_out, sd_out [n_groups][B].  `scratch`: 5 * B * (F - 1 + FB) + 2 floats,
 * 8-byte aligned.  T >= 2. */
int sfsn_gaussian_stats(const float* stft_ri, const float* fb_tbf, int B, int F, int T, int FB, float fdrc,
                        const sfsn_feature_group* groups /* host, only geometry fields are read */, int n_groups, float* mu_out,
                        float* sd_out, float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------------------
 * Deep-filter epilogue -- replaces the output re-index of SubBandSequenceModel.forward (MODEL:160-167,
 * FROZEN:259-265), deepfiltering (MODEL:315-346, FROZEN:15-39) and the reconstruction MODEL:450-472 /
 * FROZEN:588-607 (cat groups, Nyquist bin passes through, |.|).
 *     Y[b][s][f][t] = sum_{d<df} X[b][f][t-(df-1)+d] * C[d]   (zero for t-(df-1)+d < 0)
 *     C[d] = proj[t][b*N+k][((0*fc+fci)*df+d)*S+s] + i proj[t][b*N+k][((1*fc+fci)*df+d)*S+s],  f = lo + k*fc + fci
 * Groups are laid end to end from bin 0; bins not covered (>= sum N*fc, at least Nyquist) are copied.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct sfsn_df_group {
    const float* proj; /* [T][B*n_units][2*fc*df*S] */
    int n_units, fc, df;
} sfsn_df_group;

int sfsn_deepfilter(const float* stft_ri /* [B][F][T][2] */, int B, int F, int T, int S,
                    const sfsn_df_group* groups /* host */, int n_groups, float* enh_ri /* [B][S][F][T][2] */,
                    float* enh_mag /* [B][S][F][T], nullable */, int t0, int nt /* frames [t0, t0+nt) */, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Round 6: the sub-band epilogue in ONE launch -- per group the projection of the last layer's spikes (MODEL:118 `self.proj`,
 * FROZEN:125 `fc_output_layer`: sfsn_spike_proj's product) AND everything sfsn_deepfilter does with its result (MODEL:160-167,
 * 315-346, 450-474).  The coefficient tile of a (clip, 16-frame block, unit range) is formed on the int8 matrix cores, stays in LDS,
 * is written to `proj` once (the module API's last all_layer_outputs entry; NULL: not written at all) and is applied to the noisy
 * spectrum from LDS: the coefficients are never re-read from memory.  Same results, bit for bit, as sfsn_spike_proj_multi followed
 * by sfsn_deepfilter on the same arguments.  H <= 256 (spike rows of pad64(H) bytes), every P = 2*fc*df*S a multiple of 4 and <= 256;
 * SFSN_EUNSUPPORTED otherwise (issue the two calls).
 * ---------------------------------------------------------------------------------------------------- */
typedef struct sfsn_projdf_group {
    const int8_t* spikes_i8; /* [T][B*n_units][pad64(H)] int8 spikes of the group's last layer (frame 0 of the sequence) */
    const int8_t* w_packed;  /* sfsn_w3_pack(W_p [P][H]) */
    const float* w_dq;
    const float* bias;       /* [P], nullable */
    float* proj;             /* [T][B*n_units][P] coefficient rows, 16-byte aligned; NULL = not written */
    int n_units, fc, df;
} sfsn_projdf_group;
int sfsn_proj_deepfilter(const float* stft_ri /* [B][F][T][2] */, int B, int F, int T, int S, int H,
                         const sfsn_projdf_group* groups /* host */, int n_groups, float* enh_ri /* [B][S][F][T][2] */,
                         float* enh_mag /* [B][S][F][T], nullable */, int t0, int nt /* frames [t0, t0+nt) */, void* stream);
/* sfsn_gsn_layer_scan_l01 AND sfsn_proj_deepfilter of the frames [t0, t0 + nt) in ONE launch: behind the workgroups of the two layers
 * a few epilogue workgroups follow layer 1 a 16-frame tile or two behind (layer 1 publishes its int8 rows as layer 0 does; the epilogue
 * polls the counters of the layer-1 workgroups that hold its clips' rows).  Bit-identical to the two calls.
 *   The scan lists are those of sfsn_gsn_layer_scan_l01 with T = nt: their tensors start at frame t0.  The groups, the spectra and
 *   t0 / nt are those of sfsn_proj_deepfilter: their tensors start at frame 0 of the sequence, so for every group there must be one
 *   layer-1 segment with R = B * n_units and spikes_i8 = groups[i].spikes_i8 + t0 * R * pad64(H), and n_groups = n_x + n_z
 *   (SFSN_EINVAL otherwise).  Each list is checked as its own entry point checks it (x, z, layer 1, groups), then the ties.
 *   SFSN_EUNSUPPORTED wherever one of the two entry points refuses, and where a group's P = 2*fc*df*S exceeds 192.
 *   nt = 0: SFSN_OK, nothing launched.  scratch, lag, error word: as for sfsn_gsn_layer_scan_l01 (the same size function).
 *   The environment variable SFSN_L01E_WGS sets the number of epilogue workgroups (dealt over the groups by the bytes they move, at
 *   least one per job and at most one per clip). */
int sfsn_gsn_layer_scan_l01_projdf(const sfsn_scan_segment* segs_x /* host */, const sfsn_fused_x* fin_x /* host */, int n_x,
                                   const sfsn_scan_segment* segs_z /* host */, int n_z, const sfsn_scan_segment* segs1 /* host */,
                                   const sfsn_fused_input* fin1 /* host */, int H, int shared, int lag, void* scratch,
                                   size_t scratch_bytes, const float* stft_ri /* [B][F][T][2] */, int B, int F, int T, int S,
                                   const sfsn_projdf_group* groups /* host */, int n_groups, float* enh_ri /* [B][S][F][T][2] */,
                                   float* enh_mag /* [B][S][F][T], nullable */, int t0, int nt, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Streaming sessions (BASELINE configs[4]): the input history the deep filter reaches back into (MODEL:331-333: df - 1 frames
 * of the noisy spectrum).  hist [rows][D + hop] complex64, rows = B * F: frames [hop, hop + D) move to [0, D) and the `hop`
 * new frames of inp [rows][hop] are appended, in place, in one launch.  D + hop <= 16 (SFSN_EUNSUPPORTED beyond).
 * ---------------------------------------------------------------------------------------------------- */
int sfsn_hist_shift(float* hist_ri, const float* inp_ri, int rows, int D, int hop, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * cumulative_laplace_norm (FROZEN:172-202 in the form that accepts the 5-D sub-band tensor,
 * recipes/intel_ndns/spiking_fullsubnet_freeze_phase/model_low_freq_count_time.py:182-204; FROZEN's own version raises on
 * the sub-band input): every row (clip x unit) of x [T][R][I] is divided, frame by frame, by the mean of everything the row
 * has seen so far: mean[r][t] = sum_{t' <= t} sum_i x[t'][r][i] / (I * (frames_before + t + 1)), x /= mean + 2.22e-16.
 * In place.  cum_state [R] (nullable): the running sums, in/out -- a caller that feeds a sequence in pieces passes the same
 * buffer and the number of frames already seen.  scratch: T * R floats.
 * ---------------------------------------------------------------------------------------------------- */
int sfsn_cum_laplace_norm(float* x /* [T][R][I] */, int T, int R, int I, float* cum_state /* [R], nullable */,
                          int frames_before, float* scratch /* [T][R] */, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Streaming hop -- BASELINE configs[4]: `hop` new frames of B clips through the WHOLE live model (features, every GSN layer
 * of the full-band model and of the sub-band groups, projections, deep filter: MODEL:429-473 restricted to the new frames)
 * in ONE launch, with the (h, c) state of every layer (NEURON:50-62) and the deep filter's input history carried in device
 * memory between launches.  Replaces the ~15 launches the offline kernels need per hop (each costs ~4.5 us of launch
 * boundary on this hardware, which is all a one-frame hop consists of).
 *
 * One wave owns one 16-neuron tile of one layer for 16 rows and keeps that tile's weights in registers; the workgroups of
 * consecutive stages (full-band layer 0 -> ... -> sub-band layer 0, which also computes the full-band projection it needs
 * -> ... -> sub-band projection + deep filter) hand each frame over through L2 as data-tagged granules (a write-through
 * store carries the spikes AND the launch's tag; consumers poll the payload itself).
 * The recurrent product of a layer is issued before its input has arrived (it needs the previous frame only).
 * Arithmetic is that of sfsn_features / sfsn_spike_proj / sfsn_gsn_layer_scan / sfsn_deepfilter expression by expression;
 * the real-valued input product is sfsn_input_proj_f32's fp32-MFMA form with four accumulators.  That one product is NOT
 * the offline kernels' sum: sfsn_input_proj_f32 adds the chunks into one accumulator, or (64 rows and more) takes the bf16
 * three-way split.  A layer-0 membrane of a launch therefore agrees with the offline forward's within the rounding of the
 * input product, not bit for bit (tests/test_hop_edges.py: different low bits on every case; both inside the fp64 bound).
 * Everything else is bit for bit: layer 0's spikes are the offline forward's wherever no layer-0 membrane lies within that
 * rounding of the threshold, and from equal layer-0 spikes on, every spike, every membrane of the layers above and the
 * enhanced spectrum are the offline forward's bits.
 *
 * Shared or separate gate weights (sfsn_hop_desc.unshared), LayerNorm / cumulative Laplace / no normalisation, or the offline
 * Laplace / Gaussian normalisation with the clips' statistics GIVEN (feat.mu, feat.ln_w: see sfsn_hop_seq), H % 16 == 0, H <= 320, I <= 192, P <= 256 (full-band P <= 128), at most
 * SFSN_HOP_MAX_LAYERS layers and SFSN_HOP_MAX_GROUPS groups, D + hop <= 32, and few enough rows that every wave tile gets
 * its own compute unit (SFSN_EUNSUPPORTED otherwise: the caller then runs the per-kernel sequence).
 * ---------------------------------------------------------------------------------------------------- */
#define SFSN_HOP_MAX_LAYERS 3
#define SFSN_HOP_MAX_GROUPS 4
typedef struct sfsn_hop_layer {
    /* (desc.unshared: every image below covers the 2H rows of both gates, the forget gate's H rows first: [2H/16] fragment tiles,
     *  sfsn_w3_pack(W [2H][.]) and dq vectors of 2H entries) */
    const float* w_ih_frag; /* layer 0: fp32 W_ih [H][I] in MFMA fragment order [H/16][KC][64][4], KC = ceil(I/16):
                               element ((tile*KC + c)*64 + 16*q + n)*4 + e = W_ih[16*tile + n][16*c + 4*q + e], zero where
                               the column index is >= I (NULL for layers >= 1)                                      */
    const int8_t* w_ih;     /* layers >= 1: sfsn_w3_pack(W_ih [H][H]) (NULL for layer 0)                            */
    const float* w_ih_dq;
    const int8_t* w_hh;     /* sfsn_w3_pack(W_hh [H][H])                                                            */
    const float* w_hh_dq;
    const float* bias;      /* [2H] bias_ih                                                                         */
    const float* bn_alpha;  /* [H]                                                                                  */
    const float* bn_beta;   /* [H]                                                                                  */
    int8_t* h[2];           /* [R][pad64(H)] x 2: spikes of the last frame, in/out; launch k (= launch_index) reads
                               h[k & 1] and writes h[(k + 1) & 1]; zero both to reset                                 */
    float* c;               /* [R][H] membrane, in/out                                                              */
    int8_t* spikes;         /* [hop][R][pad64(H)] scratch, zeroed by the caller once (bit 0 of a byte = the spike,
                               bits 1..7 = the tag of the launch that wrote it)                                      */
} sfsn_hop_layer;
typedef struct sfsn_hop_seq {      /* one sequence model: the full-band model or one sub-band group                  */
    sfsn_hop_layer layer[SFSN_HOP_MAX_LAYERS];
    int n_layers, H, P;
    sfsn_feature_group feat;       /* geometry + normalisation of this model's input rows (`x` unused); rows R = B * feat.n_units,
                                      row b * n_units + k.  SFSN_NORM_LAPLACE: `mu` = [B] device floats, the clips' means, GIVEN by
                                      the caller (a calibration pass, an earlier utterance, sfsn_laplace_means of the clip itself):
                                      y = v / (mu[b] + 2.220446049250313e-16f), sfsn_features' expression; mu == NULL answers
                                      SFSN_EUNSUPPORTED (utterance statistics the launch would have to compute are not causal).
                                      SFSN_NORM_GAUSSIAN: `mu` = [B] means and `ln_w` = [B] standard deviations,
                                      y = (v - mu[b]) / (ln_w[b] + 2.220446049250313e-16f); either NULL: SFSN_EINVAL.  Both must be
                                      4-byte aligned (SFSN_EINVAL).  Every launch reads them; nothing of them is carried in the state.
                                      Given statistics run kernels of their own: in one descriptor they go with each other and
                                      with SFSN_NORM_NONE, not with LayerNorm / the cumulative norm (SFSN_EUNSUPPORTED)          */
    const int8_t* w_p;             /* sfsn_w3_pack(proj.weight [P][H])                                               */
    const float* w_p_dq;
    const float* b_p;              /* [P]                                                                            */
    int df;                        /* deep-filter order of a sub-band group; 0 for the full-band model               */
    int fc;                        /* sub-band group: centre bins per unit (P == 2 * fc * df * S)                    */
    float* cum[2];                 /* feat.norm == SFSN_NORM_CUMLAPLACE: [R] x 2, the rows' running sums, in/out (launch k reads
                                      cum[k & 1], writes cum[(k + 1) & 1]; zero both to reset); NULL otherwise          */
} sfsn_hop_seq;
typedef struct sfsn_hop_desc {
    sfsn_hop_seq fb;
    sfsn_hop_seq sb[SFSN_HOP_MAX_GROUPS];
    int n_groups;
    int B, F, S, hop, D;           /* D = max(df) - 1 frames of history                                              */
    float fdrc;
    const float* inp_ri;           /* [B][F][hop][2] the new noisy frames                                            */
    float* hist_ri;                /* [B][F][D][2]   the last D noisy frames, in/out (zero to reset); NULL if D == 0 */
    float* enh_ri;                 /* [B][S][F][hop][2] out                                                          */
    float* enh_mag;                /* [B][S][F][hop] out, nullable                                                   */
    void* scratch;                 /* sfsn_hop_scratch_bytes(desc) bytes, ZEROED by the caller once; word 0 = error flag
                                      (non-zero after a launch: a bounded hand-off wait expired, results invalid)     */
    size_t scratch_bytes;
    unsigned launch_index;         /* launches made on this state so far: the caller adds 1 after every launch (it picks
                                      the hand-off tag and the parity of the double-buffered state; a launch must not
                                      be replayed with the index of its predecessor, so no graph capture)            */
    /* Waveform mode (hop == 1, n_fft 512 / hop_length 128; wave_in != NULL): the launch also computes the new frame's
     * spectrum from the samples (torch.stft(center=True) framing: the frame that ends with these 128 samples, i.e. frame
     * frame_index of the utterance when the caller has fed 128 * (frame_index + 2) samples) and turns the enhanced frame back
     * into samples (torch.istft's overlap-add and envelope): wave_out receives the 128 padded positions
     * [128 * frame_index, 128 * frame_index + 128), i.e. output samples [128 * (frame_index - 2), 128 * (frame_index - 1)) --
     * the first two launches of an utterance write the part torch.istft trims.  inp_ri is ignored. */
    const float* wave_in;          /* [B][128] the new samples                                                       */
    float* wave_state;             /* [B][512] the last 512 input samples, in/out (zero = start of an utterance)      */
    float* ola_state;              /* [B][S][512] overlap-add accumulator of the output, in/out (zero to reset)       */
    float* wave_out;               /* [B][S][128] out                                                                */
    const float* window;           /* [512] analysis / synthesis window (the reference: hann)                       */
    float* spec_g;                 /* [B][F][4] scratch ({re, tag, im, tag} granules of the noisy frame), zeroed once */
    float* enh_g;                  /* [B][S][F][4] scratch (granules of the enhanced frame), zeroed once              */
    int frame_index;
    unsigned* done;                /* nullable, [B][S]: word (b, s) is set to launch_index + 1 (system-scope release) once wave_out
                                      (b, s) has been written.  wave_in, wave_out and done may be pinned host memory the device can
                                      reach: samples in host memory -> enhanced samples in host memory with no copy launch and no
                                      stream synchronisation (the caller spins on the words)                               */
    int frames_before;             /* frames this state has seen since it was zeroed (the caller adds `hop` after every launch):
                                      SFSN_NORM_CUMLAPLACE's denominator                                             */
    int unshared;                  /* non-zero: separate forget / cell gate weights (shared_weights = False, NEURON:137-139): every
                                      layer's w_hh / w_ih images and dq vectors cover 2H rows, forget rows first (ABI 15)      */
    const unsigned* clip_start;    /* nullable, [B] (ABI 20): per-clip utterances.  clip_start[b] = the launch index at which clip b's
                                      utterance began (its frame 0); the launch with index k gives clip b frame index k - clip_start[b]
                                      and (k - clip_start[b]) * hop frames before it (unsigned differences: wrap-safe) instead of
                                      frame_index / frames_before.  In the launch k == clip_start[b] every stage reads clip b's
                                      carried state as zero (h, c, cum, hist_ri, ola_state) instead of loading it, so that one clip
                                      restarts while the others go on.  Waveform mode: in the launch k == clip_start[b] - 1 (the
                                      clip's first call, no frame yet) the STFT stage leaves [0 x 384 | the new samples] in the clip's
                                      wave_state; wave_out of clip b is zero while its frame index is < 2.  The caller writes an entry
                                      only where no launch that is already queued reads it (a stream-ordered fill); the resident
                                      kernel reads the array (then pinned host memory) after each doorbell.  NULL: the session-wide
                                      frame_index / frames_before, no restarts                                            */
    unsigned* spike_slots;         /* nullable, sfsn_hop_spike_slots(desc) words (ABI 21): running spike counts, zeroed by the caller
                                      to reset.  Layout: the full-band model, then groups 0 .. n_groups - 1; within a sequence layer
                                      by layer; within a layer [R][H / 4]: slot (row, j) counts the spikes of neurons 4j .. 4j + 3 of
                                      row `row` (clip row / feat.n_units).  One lane of the launch owns each slot and adds, once per
                                      launch, the spikes of the `hop` frames it computed (plain per-lane load + store: no atomics).
                                      With clip_start: in the launch that restarts the row's clip the slot reads as zero instead of
                                      being loaded; in a waveform clip's first call (no frame yet) the slot is written as zero.  May be
                                      pinned host memory: the resident kernel writes a hop's slots before it releases that hop's done
                                      words, so the host may read them for every hop whose done words it has seen.  NULL: no counting */
} sfsn_hop_desc;

size_t sfsn_hop_scratch_bytes(const sfsn_hop_desc* desc /* host */);
/* Words of desc->spike_slots: sum over the sequences and their layers of R * H / 4 (0 for a descriptor the launch refuses). */
size_t sfsn_hop_spike_slots(const sfsn_hop_desc* desc /* host */);
int sfsn_stream_hop(const sfsn_hop_desc* desc /* host */, void* stream);

/* sfsn_stream_hop with HELD clips: bit b of held_bits (ceil(B / 64) words, host memory, read before the call returns) = clip b has
 * no frame this tick and sits launch k = desc->launch_index out.  ONE launch and nothing else on the stream: the mask travels by value
 * in the kernel arguments (no device buffer a queued launch could find overwritten, no copy enqueued).  held_bits == NULL or all bits
 * zero IS sfsn_stream_hop: the same kernels, which do not carry the predicate (the held form is a template instantiation of its own).
 * Every stage, hand-off and tag runs as in sfsn_stream_hop -- rows are independent in every product, LayerNorm and filter, so a held
 * clip's rows compute on whatever inp_ri / wave_in hold for them (anything, NaN included; nothing of it reaches another clip or any
 * carried state) and no wait is added.  For a row of a held clip b:
 *   h          h[(k + 1) & 1] <- the bytes of h[k & 1] (instead of the new spikes);
 *   c          not written;          spike_slots   not added to (nor zeroed);
 *   cum        cum[(k + 1) & 1] <- cum[k & 1], no row sum added;
 *   hist_ri    not shifted;
 *   wave_state not shifted, and a first call (k == clip_start[b] - 1) does not take the samples;   ola_state not touched;
 *   enh_ri, enh_mag, wave_out   written as zero;      done   written (launch_index + 1), so a host that waits on the words returns;
 *   clip_start[b] += 1 (unsigned): the clip's origin moves on by one launch, so that launch k + 1 -- and sfsn_hop_prime / _seed /
 *              _advance / _state_export, which all read clip b through its origin -- see it exactly as if launch k had never happened
 *              for it: same frame index, same frames_before, and a restart or first call that was due in launch k is due in k + 1.
 * The origin rule: the + 1 is ordered after every read of clip_start in this launch and before the next launch on the stream.  It is
 * done in the launch: each workgroup, its role finished, adds 1 to word 3 of `scratch` (vector atomic) as its last act, and the
 * workgroup that finds itself last applies the + 1s and clears the word.  Nobody waits on that word: no spin is added.  clip_start
 * must therefore be device-writable memory the caller hands over for the launch (the caller still numbers the launches itself and
 * adds 1 to launch_index after this one too).  The caller's own bookkeeping of a held clip's frames / calls does not advance.
 * Returns what sfsn_stream_hop returns for the descriptor (a descriptor it refuses: the same code); with some bit set:
 *   a bit at or beyond desc->B                          SFSN_EINVAL
 *   desc->clip_start == NULL                            SFSN_EINVAL   (a held clip needs an origin of its own)
 *   desc->B > 256 (what the argument block carries)     SFSN_EUNSUPPORTED
 * Not for the resident form.  The cIRM-GSN hop has its own held entries: sfsn_fullband_stream_hop_held / _wave_held. */
int sfsn_stream_hop_held(const sfsn_hop_desc* desc /* host */, const uint64_t* held_bits /* host, ceil(B/64) words, bit b = clip b is held */, void* stream);

/* ---- Outer samples: three times the model's rate and / or 16-bit PCM (additive exports; the ABI version stays 21) -------------------
 * One linear-phase low-pass h[0 .. 95], given by the caller as float32 (the package: sinc((k - 47.5) / 3) / 3 * kaiser(96, 8)[k],
 * normalised to sum 1 in float64, then rounded), serves both ways:
 *   down (3 -> 1)   y[m] = sum_{k = 0 .. 95} taps[k] x[3 m + 2 - k],          x[n < 0] = the carried samples (zero at the start);
 *   up   (1 -> 3)   z[3 m + p] = sum_{j = 0 .. 31} phase_taps[32 p + j] y[m - j],   phase_taps[32 p + j] = 3 h[3 j + p] (rounded once).
 * Summation order (the stand-alone kernels and the hop give the same bits): ONE fp32 accumulator from 0.0f, fmaf, ascending k (j).
 * Carried state: down, per row 96 floats -- the last 93 input samples as float32, oldest first, 3 words of padding (written zero);
 *                up, per row 32 floats -- the last 31 values of y, oldest first, one word of padding.
 * Formats: SFSN_SAMPLE_F32; SFSN_SAMPLE_S16 in: (float)s * 2^-15 (exact); out: clamp(rintf(v * 32768), -32768, 32767), ties to even,
 * NaN -> 0.  Strides count samples of the buffer's own format. */
#define SFSN_SAMPLE_F32 0
#define SFSN_SAMPLE_S16 1
/* in: B rows of 3 n_out samples of in_format, row b at in + b * in_stride samples (in_stride >= 3 n_out; what lies between rows is never
 * read); out: float32 [B][n_out]; state: [B][96] read and updated in place, or NULL = zeros and nothing carried.  A signal fed in
 * chunks with its state carried gives the bits of one call.  SFSN_EINVAL, in this order: an unknown format; a NULL in / taps / out,
 * B or n_out < 1, in_stride < 3 n_out.  Both refusals are answered without a device. */
int sfsn_resample_down3(const void* in, int in_format, int B, int n_out, long long in_stride, const float* taps /* [96] */,
                        float* state /* [B][96], nullable */, float* out /* [B][n_out] */, void* stream);
/* in: float32 [R][n_in]; out: R rows of 3 n_in samples of out_format, row r at out + r * out_stride samples (only those 3 n_in are
 * written); state: [R][32] read and updated in place, or NULL.  Refusals as above (out_format first). */
int sfsn_resample_up3(const float* in /* [R][n_in] */, int R, int n_in, const float* phase_taps /* [3][32] */, float* state /* [R][32], nullable */,
                      void* out, int out_format, long long out_stride, void* stream);

/* sfsn_stream_hop / sfsn_stream_hop_held for a waveform descriptor whose OUTER samples differ from the model's: the conversion runs in
 * the launch's first and last stage, by the waves that build the frame and that finish the inverse STFT -- no further launch, wait,
 * hand-off, tag or workgroup. */
typedef struct {
    int ratio;                /* outer rate / model rate: 1 or 3 (128 * ratio samples per clip and launch, each way)               */
    int format;               /* SFSN_SAMPLE_*: the format of wave_in AND wave_out                                                 */
    const void* wave_in;      /* [B][128 * ratio] the new outer samples (may be pinned host memory, like desc->wave_in)            */
    void* wave_out;           /* [B][S][128 * ratio] out (may be pinned host memory)                                               */
    float* dec_state;         /* [B][96]    the decimator's carried samples, in/out (zero = start of an utterance); ratio 3 only    */
    float* int_state;         /* [B][S][32] the interpolator's carried samples, in/out; ratio 3 only                              */
    const float* taps;        /* [96]; ratio 3 only                                                                                */
    const float* phase_taps;  /* [3][32]; ratio 3 only                                                                             */
} sfsn_hop_io;
/* io == NULL IS sfsn_stream_hop_held(desc, held_bits, stream) (and with held_bits == NULL, sfsn_stream_hop).  Otherwise desc->wave_in and
 * desc->wave_out are ignored and the launch
 *   reads   io->wave_in; every clip's dec_state row (as zero in the clip's first call of an utterance, k == clip_start[b] - 1, which is
 *           how a restart reaches the filter with no extra launch); every pair's int_state row; taps, phase_taps; all sfsn_stream_hop reads;
 *   writes  io->wave_out: U3(the 128 samples sfsn_stream_hop would have written) in io->format, stored before the pair's done word;
 *           ZERO while the pair's frame index is < 2 (with or without clip_start -- the two hops torch.istft trims), and int_state is
 *           then written as zero: the interpolator sees the zeros its caller sees;
 *           wave_state [B][512]: the last 512 samples at the MODEL's rate, D3(io->wave_in) appended; dec_state: the last 93 outer samples;
 *           everything else sfsn_stream_hop writes.
 *   held    (bit b of held_bits) as sfsn_stream_hop_held, and: dec_state and int_state of the clip are not touched, io->wave_out of the
 *           clip is zero in io->format.
 * ratio 1 with SFSN_SAMPLE_F32 launches the kernels of sfsn_stream_hop(_held) on io's buffers; the other three combinations have
 * instantiations of their own, in which the plain kernels' code is unchanged.  Returns, in this order:
 *   io->ratio not 1 or 3                                   SFSN_EINVAL
 *   io->format unknown                                     SFSN_EINVAL
 *   desc NULL or not a waveform descriptor (wave_state)    SFSN_EINVAL
 *   desc->hop != 1                                         SFSN_EUNSUPPORTED
 *   a NULL io->wave_in / wave_out; ratio 3: a NULL state or tap pointer   SFSN_EINVAL
 * then whatever sfsn_stream_hop_held returns.  All of these are answered without a device.  Not for the resident form. */
int sfsn_stream_hop_io(const sfsn_hop_desc* desc /* host */, const sfsn_hop_io* io /* host, nullable */, const uint64_t* held_bits /* nullable */,
                       void* stream);

/* The RESIDENT form of the waveform hop (BASELINE.json configs[4] names a "persistent kernel"; round 3).  One launch serves hop
 * after hop of a waveform session with host completion words (wave_in, wave_out and done in pinned host memory, hop == 1):
 * for hop k = 0, 1, ... the host writes the 128 samples per clip into wave_in, then stores k + 1 into the 32-bit `doorbell`
 * word (pinned host memory too), then waits until every done word reads desc->launch_index + k + 1 -- only then may it ring
 * hop k + 1.  The kernel uses launch index desc->launch_index + k, frame index desc->frame_index + k and
 * desc->frames_before + k for hop k (what k separate sfsn_stream_hop calls would have been given).  Storing 0xFFFFFFFF ends the
 * kernel; so does a doorbell silent for about `idle_ms` milliseconds and an expired hand-off wait (error word set, as for a
 * launch): the kernel never outlives its caller by more than that.  The caller keeps `stream` free of other work while
 * the kernel is resident (it holds the hop's workgroups -- 23 of 256 CUs for the M model at B = 1) and adds the hops served to
 * its own launch / frame counters afterwards; doorbell[1] (zeroed by the caller before the call) is set to 1 by the kernel when it
 * leaves.  Same results as the launches, bit for bit.  desc->clip_start, if set, may be pinned host memory: hop k reads it after
 * its doorbell, so the host may change entries for hop k + 1 once hop k's done words are in and before it rings hop k + 1. */
int sfsn_stream_hop_resident(const sfsn_hop_desc* desc /* host */, void* doorbell /* pinned host, u32[2] */, unsigned idle_ms,
                             void* stream);
/* Diagnostic: the launch's stages in block order, out[4 * i] = {sequence (0 = full-band, 1 + g = group g), layer (-1 = projection
 * [+ deep filter]), first workgroup, workgroups}; returns the number of stages (or a negative status).  With SFSN_HOP_DEBUG set
 * in the environment a launch leaves eight 100 MHz time stamps per wave (4 waves per workgroup) in `scratch`, behind the
 * 64 bytes of control words: entry, set-up done, recurrent half issued, full-band projection arrived (sub-band layer 0),
 * input arrived, frame computed, deep filter done, exit (scripts/exp_hop.py prints them per stage). */
int sfsn_hop_stages(const sfsn_hop_desc* desc /* host */, int* out /* host [cap][4] */, int cap);

/* Priming (csrc/sfsn_prime.hip): the state N / hop launches of sfsn_stream_hop on a recorded prefix of N frames would have left, written
 * in ONE launch from what the OFFLINE kernels computed for that prefix -- for the listed clips of the descriptor only; every other
 * clip's rows, the tagged scratch (spikes, spec_g, enh_g) and launch_index are left as they are.  `src` describes tensors of Bp clips;
 * clips[i] (an index of desc's batch, distinct, n_clips >= 1) takes the prefix of source clip b0 + i.  With k = desc->launch_index:
 *   layer.h[k & 1]  <- the last frame's spikes (row N - 1 of spikes_i8), layer.c <- the membrane (c), in the hop's row layout;
 *   cum[k & 1]      <- the rows' running sums (sfsn_cum_laplace_norm's cum_state: the hop adds the same row sums in the same order);
 *   hist_ri         <- the last D noisy frames of the bins the groups cover (zeros before the prefix's first frame);
 *   spike_slots     <- slot (row, j) = the spikes of neurons 4j .. 4j + 3 of `row` over the N frames (REPLACED, not added to);
 *   wave_state      <- wave_tail, the last 512 input samples; ola_state <- the overlap-add partial sums the last three frames of enh_ri
 *                      leave for the padded positions not yet emitted (sfsn_hop_wave_dev.h's arithmetic in ascending frame order).
 * The caller then sets clip_start[clips[i]] = k - N / hop (unsigned, wrap-safe): launch k gives those clips frame index N / hop and reads
 * the state above.  An origin equal to k would make launch k read the state as ZERO -- which is what N = 0 means (waveform mode only:
 * a clip whose one call of samples has made no frame yet; everything but wave_state is written as zero).
 * Bit for bit what the launches would have left wherever the offline forward and the hop agree bit for bit (see above: all but layer
 * 0's membranes, which are the offline forward's here).  Plain stores, no atomics; ordered on `stream` like any launch.
 * SFSN_EINVAL: NULL desc / clips / src, n_clips < 1, an index outside [0, desc->B) or listed twice, N % hop != 0, N < hop (waveform
 * mode: N < 0), b0 + n_clips > Bp, a missing or misaligned source pointer (c: 16 bytes; stft_ri, enh_ri: 8; the others: 4).
 * SFSN_EUNSUPPORTED: a descriptor sfsn_stream_hop refuses, more than 256 listed clips (prime them in several calls). */
typedef struct sfsn_prime_layer {
    const int8_t* spikes_i8; /* [N][Bp * n_units][pad64(H)] the layer's int8 spikes of the prefix (bytes 0 / 1) */
    const float* c;          /* [Bp * n_units][H] its membrane after frame N - 1 (c_state)                      */
} sfsn_prime_layer;
typedef struct sfsn_prime_seq {
    sfsn_prime_layer layer[SFSN_HOP_MAX_LAYERS];
    const float* cum;        /* SFSN_NORM_CUMLAPLACE: [Bp * n_units] the running sums after frame N - 1; NULL otherwise */
} sfsn_prime_seq;
typedef struct sfsn_prime_src {
    int Bp, N, b0;
    const float* stft_ri;    /* [Bp][F][N][2] the noisy prefix (NULL if D == 0 or N == 0)                     */
    const float* enh_ri;     /* waveform mode: [Bp][S][F][N][2] the enhanced prefix (NULL if N == 0)           */
    const float* wave_tail;  /* waveform mode: [Bp][512] the last 512 input samples, zeros in front of a shorter input */
    sfsn_prime_seq fb;
    sfsn_prime_seq sb[SFSN_HOP_MAX_GROUPS];
} sfsn_prime_src;
int sfsn_hop_prime(const sfsn_hop_desc* desc /* host */, const int* clips /* host */, int n_clips, const sfsn_prime_src* src /* host */,
                   void* stream);

/* A backlog on a clip that is ALREADY RUNNING (csrc/sfsn_prime.hip): N new frames through the OFFLINE kernels, started from the state
 * the session carries instead of from zero, and their end state handed back -- what N / hop launches of sfsn_stream_hop would have
 * computed and left, at offline speed.  Two launches around the offline kernels, for the listed clips of the descriptor only
 * (distinct indices, 1 <= n_clips <= 256); every other clip's rows, the tagged scratch (spikes, spec_g, enh_g) and launch_index are
 * left as they are.  Plain loads and stores, no atomics, nothing waits; ordered on `stream` like any launch.  k = desc->launch_index.
 *
 * sfsn_hop_seed: the offline kernels' START tensors, rows b0 + i of tensors of Bp clips for clips[i]:
 *   layer.h   <- h[k & 1] as fp32 0 / 1 [Bp * n_units][H] (a scan's h_state), layer.c <- c (its c_state);
 *   cum       <- cum[k & 1], the rows' running sums (sfsn_cum_laplace_norm's cum_state; its frames_before is (k - clip_start) * hop);
 *   stft_ri   <- frames [0, D) of every row [F][T][2] = hist_ri, the last D noisy frames (zeros for the bins the hop keeps no history
 *                of: no group covers them, nobody reads them).  The caller puts the N new frames at [T - N, T), T >= D + N, and runs
 *                the offline stages on those frames of the buffer, so that the deep filter reaches back into real history;
 *   wave_ctx  <- waveform mode: wave_state[128 .. 512), the 384 samples the next frame begins with, at the front of a row of
 *                wave_stride floats (the caller appends the new samples: frame j of the backlog is the centred frame j + 2 of that
 *                row on sfsn_stft).
 * desc->clip_start is read: a clip whose origin equals k (a restarted or never-stepped clip: the hop reads its state as zero in launch
 * k, whatever memory holds) is written as zeros everywhere but wave_ctx (its first call has left [0 x 384 | samples] in wave_state).
 *
 * sfsn_hop_advance: the continuing form of sfsn_hop_prime.  `src` holds the offline kernels' results for the N new frames:
 *   layer.h[k & 1], layer.c, cum[k & 1] <- row N - 1 of spikes_i8, c, cum (the end state of the backlog);
 *   hist_ri     <- the last D frames of stft_ri's rows of T frames, [history | new]: N < D keeps the tail of the old history;
 *   spike_slots <- ADDED to: slot (row, j) += the spikes of neurons 4j .. 4j + 3 of `row` over the N frames (a clip whose origin
 *                  equals k: replaced, the hop reads its slot as zero);
 *   wave_state  <- wave_tail, the last 512 input samples; ola_state <- continued in the hop's order: the carried partial sums first
 *                  (zero for a clip whose origin equals k), then frames T - N .. T - 1 of enh_ri's rows in ascending order
 *                  (sfsn_hop_wave_dev.h's arithmetic and envelope); wave_out[b0 + i][s][128 j ..] <- the block launch k + j would
 *                  have written (zero while the clip's frame index k + j - clip_start is < 2).
 * The caller then moves clip_start[clips[i]] back by N / hop (unsigned, wrap-safe) with a stream-ordered device operation behind the
 * queued launches: launch k continues at the clip's frame index + N / hop.  For a clip whose origin was k that is k - N / hop,
 * sfsn_hop_prime's formula.  clip_start == NULL: no clip is fresh, frame indices come from desc->frame_index.
 *
 * Exactness: sfsn_hop_prime's one reservation and no other.  The layer-0 membranes written back are the offline kernels', which
 * differ from the hop's in their low bits (the layer-0 input product sums in another association).  Where no layer-0 membrane of the
 * backlog lies within that rounding of the threshold, every spike, every higher-layer membrane, every output and every count is that
 * of the launch sequence, bit for bit.
 * SFSN_EINVAL, before any launch: a NULL desc / clips / dst / src, n_clips < 1, an index outside [0, desc->B) or listed twice,
 * b0 + n_clips > Bp, N % hop != 0, N < hop, T < D + N (seed: T < D), wave_stride < 384, a missing or misaligned pointer (h, c: 16
 * bytes; stft_ri, enh_ri, wave_out: 8; the others: 4).  SFSN_EUNSUPPORTED: a descriptor sfsn_stream_hop refuses, more than 256
 * listed clips (the caller splits the list), B > 65535.  (Added without an ABI bump: no existing struct or signature changed.) */
typedef struct sfsn_seed_layer {
    float* h;                /* [Bp * n_units][H] fp32 0 / 1 */
    float* c;                /* [Bp * n_units][H]            */
} sfsn_seed_layer;
typedef struct sfsn_seed_seq {
    sfsn_seed_layer layer[SFSN_HOP_MAX_LAYERS];
    float* cum;              /* SFSN_NORM_CUMLAPLACE: [Bp * n_units]; NULL otherwise */
} sfsn_seed_seq;
typedef struct sfsn_seed_dst {
    int Bp, T, b0;
    int wave_stride;         /* waveform mode: floats per row of wave_ctx (>= 384)                   */
    float* stft_ri;          /* [Bp][F][T][2]: frames [0, D) are written (NULL if D == 0)            */
    float* wave_ctx;         /* waveform mode: [Bp][wave_stride], samples [0, 384) are written       */
    sfsn_seed_seq fb;
    sfsn_seed_seq sb[SFSN_HOP_MAX_GROUPS];
} sfsn_seed_dst;
typedef struct sfsn_advance_src {
    int Bp, N, b0;
    int T;                   /* frames per row of stft_ri / enh_ri; the N new frames are the last ones  */
    const float* stft_ri;    /* [Bp][F][T][2] [history | new] (NULL if D == 0)                          */
    const float* enh_ri;     /* waveform mode: [Bp][S][F][T][2] the enhanced frames                     */
    const float* wave_tail;  /* waveform mode: [Bp][512] the last 512 input samples                     */
    float* wave_out;         /* waveform mode: [Bp][S][128 * N] out                                     */
    sfsn_prime_seq fb;       /* spikes_i8: the N new frames' [N][Bp * n_units][pad64(H)]; c, cum: after the last one */
    sfsn_prime_seq sb[SFSN_HOP_MAX_GROUPS];
} sfsn_advance_src;
int sfsn_hop_seed(const sfsn_hop_desc* desc /* host */, const int* clips /* host */, int n_clips, const sfsn_seed_dst* dst /* host */,
                  void* stream);
int sfsn_hop_advance(const sfsn_hop_desc* desc /* host */, const int* clips /* host */, int n_clips, const sfsn_advance_src* src /* host */,
                     void* stream);

/* sfsn_hop_advance with a backlog of ITS OWN LENGTH per clip (csrc/sfsn_prime.hip): the offline kernels ran ONE padded forward of Nmax
 * new frames behind lead = T - Nmax >= D frames of history (a ragged batch, the padding zeroed), clip b0 + i has N_b = frames[b0 + i]
 * of them (device int32 [Bp], each a multiple of hop with hop <= N_b <= Nmax: the CALLER's check -- the launch holds a value outside
 * [1, Nmax] inside that range, so that no index leaves the tensors, and promises nothing else about such a clip).  For clips[i], with
 * k = desc->launch_index:
 *   layer.h[k & 1] <- row N_b - 1 of spikes_i8; layer.c <- row N_b - 1 of `membrane`, the post-BatchNorm membrane of every frame
 *                     (sfsn_scan_segment.membrane: the value that becomes c_state behind the last frame of a scan -- c_state itself is
 *                     the membrane after the last PADDED frame and is not read);
 *   hist_ri        <- the D frames that end with frame lead + N_b - 1 of stft_ri's row, [history | new]: N_b < D keeps the tail of the old
 *                     history;
 *   spike_slots    <- ADDED to over frames [0, N_b) only (a clip whose origin equals k: replaced);
 *   wave_state     <- the 512 samples that end at sample 384 + 128 N_b of the clip's row of wave_ctx ([384 of context | new samples],
 *                     the row sfsn_hop_seed began); ola_state <- continued in the hop's order through frame N_b - 1 only;
 *                     wave_out[b0 + i][s][128 j ..] <- block j < N_b as sfsn_hop_advance writes it, zeros for N_b <= j < Nmax.
 * The caller then moves clip_start[clips[i]] back by ITS OWN N_b / hop with a stream-ordered device operation behind the queued
 * launches.  Everything else -- the untouched clips and scratch, fresh clips, clip_start == NULL, the exactness reservation (layer 0's
 * membranes are the offline kernels') -- is sfsn_hop_advance's.  A descriptor with SFSN_NORM_CUMLAPLACE is refused
 * (SFSN_EUNSUPPORTED): the sub-band running sums after a clip's own last frame are not available from a padded forward; make one
 * sfsn_hop_advance call per length.
 * SFSN_EINVAL, before the launch: as sfsn_hop_advance with Nmax in the place of N (Nmax % hop != 0, Nmax < hop, T < D + Nmax), a missing
 * or misaligned pointer (membrane: 16 bytes; stft_ri, enh_ri, wave_out: 8; frames, spikes_i8, wave_ctx: 4), wave_stride < 384 +
 * 128 Nmax.  SFSN_EUNSUPPORTED: as sfsn_hop_advance, and the cumulative norm.  (Added without an ABI bump: a new function and new
 * structs only.) */
typedef struct sfsn_ragged_layer {
    const int8_t* spikes_i8; /* [Nmax][Bp * n_units][pad64(H)] the new frames' int8 spikes (bytes 0 / 1)  */
    const float* membrane;   /* [Nmax][Bp * n_units][H] the new frames' post-BatchNorm membranes          */
} sfsn_ragged_layer;
typedef struct sfsn_ragged_seq {
    sfsn_ragged_layer layer[SFSN_HOP_MAX_LAYERS];
} sfsn_ragged_seq;
typedef struct sfsn_advance_ragged_src {
    int Bp, Nmax, b0;
    int T;                   /* frames per row of stft_ri / enh_ri; the Nmax (padded) new frames are the last ones */
    int wave_stride;         /* waveform mode: floats per row of wave_ctx (>= 384 + 128 Nmax)                      */
    const int* frames;       /* DEVICE int32 [Bp]: N_b, the new frames clip b0 + i really has                      */
    const float* stft_ri;    /* [Bp][F][T][2] [history | new | padding] (NULL if D == 0)                           */
    const float* enh_ri;     /* waveform mode: [Bp][S][F][T][2] the enhanced frames                                */
    const float* wave_ctx;   /* waveform mode: [Bp][wave_stride] 384 samples of context, then the new samples      */
    float* wave_out;         /* waveform mode: [Bp][S][128 * Nmax] out                                             */
    sfsn_ragged_seq fb;
    sfsn_ragged_seq sb[SFSN_HOP_MAX_GROUPS];
} sfsn_advance_ragged_src;
int sfsn_hop_advance_ragged(const sfsn_hop_desc* desc /* host */, const int* clips /* host */, int n_clips,
                            const sfsn_advance_ragged_src* src /* host */, void* stream);

/* Moving a clip (csrc/sfsn_state.hip): the carried state of the listed clips out into a self-contained blob per clip, and from such a
 * blob into the listed clips of this or another descriptor of the same geometry -- ONE launch each way, ordered on `stream` like any
 * launch, plain stores, nothing waits inside it.  The state is COPIED, not recomputed, so a moved clip continues bit for bit, layer 0
 * included (priming has a reservation there).  Every other clip's rows, the tagged scratch (spikes, spec_g, enh_g) and launch_index are
 * left as they are.  With k = desc->launch_index, export READS and import WRITES the half of every double-buffered array that launch k
 * reads (h[k & 1], cum[k & 1]); the two descriptors' parities may differ -- the blob has none.
 *
 * Blob of sfsn_hop_state_export: one clip = sfsn_hop_state_bytes(desc) bytes, blob row i = clips[i] (import: row b0 + i -> clips[i]).
 * Sections in this order, each starting at the next multiple of 16 bytes, the total rounded up to a multiple of 16:
 *   for every sequence (the full-band model, then groups 0 .. n_groups - 1) and every layer of it, with units = feat.n_units:
 *       h      int8  [units][H]      the last frame's spike bytes (the pad columns H .. pad64(H) - 1 of the session's rows are not state)
 *       c      float [units][H]      the membranes
 *   cum        float [units]         for every sequence with SFSN_NORM_CUMLAPLACE, in sequence order: the rows' running sums
 *   slots      u32   [units][H / 4]  only if desc->spike_slots: for every sequence and layer, in that order
 *   hist       float [fcov][D][2]    only if D > 0: the last D noisy frames of the bins 0 .. fcov - 1 the groups cover
 *                                    (fcov = max over groups of feat.lo + feat.n_units * fc; the hop keeps no history of the others)
 *   wave       float [512]           only in waveform mode (wave_in != NULL): wave_state, the last 512 input samples
 *   ola        float [S][512]        only in waveform mode: ola_state
 * sfsn_hop_state_bytes is host only (no device needed) and returns 0 for a descriptor sfsn_stream_hop refuses.
 *
 * The clip's ORIGIN is not in the blob: it is not device state of the hop, clip_start is the caller's array.  At export the caller
 * notes age = launch_index - clip_start[b] of the source (unsigned difference); after an import it writes, with a stream-ordered fill
 * behind the queued launches, clip_start[b'] = launch_index - age of the destination (unsigned, wrap-safe).  age may be -1 (a waveform
 * clip that has not made its first call yet: its origin is the launch after the destination's next one) and may exceed the
 * destination's launch_index.  age == 0 makes the next launch read the state as zero, which is then what it is.
 *
 * SFSN_EINVAL, before any launch: NULL desc / clips / blob, n_clips < 1, an index outside [0, desc->B) or listed twice, b0 < 0, a blob
 * pointer that is not 16-byte aligned, a NULL or 4-byte-misaligned state pointer.  SFSN_EUNSUPPORTED: more than 256 clips (the caller
 * splits the list), B > 65535, a descriptor sfsn_stream_hop refuses.
 * (Added without an ABI bump: no existing struct or signature changed.) */
size_t sfsn_hop_state_bytes(const sfsn_hop_desc* desc /* host */);
int sfsn_hop_state_export(const sfsn_hop_desc* desc /* host */, const int* clips /* host */, int n_clips,
                          void* blob /* device [n_clips][bytes] */, void* stream);
int sfsn_hop_state_import(const sfsn_hop_desc* desc /* host */, const int* clips /* host */, int n_clips,
                          const void* blob /* device [..][bytes] */, int b0 /* first blob row */, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Spike counts -- the only thing the reference's energy proxy reads from the spike tensors:
 * compute_synops (audiozen/metric.py:303-327) uses torch.gt(layer_output, 0).float().mean() per layer.  Counting the
 * int8 spikes the scan already writes lets a caller that only wants SynOPs skip the fp32 spike tensors
 * (spikes_f32 = NULL in sfsn_gsn_layer_scan): 4 B/spike of HBM writes and a 3-pass torch reduction less.
 *     *count += #{ spikes_i8[i] != 0, i < n_bytes }       (exact integer; pad columns of the int8 layout are zero)
 * One launch for up to SFSN_MAX_COUNT_TENSORS tensors.  `count` is accumulated (the caller zeroes it).
 * ---------------------------------------------------------------------------------------------------- */
#define SFSN_MAX_COUNT_TENSORS 16
typedef struct sfsn_count_tensor {
    const int8_t* spikes_i8;     /* device, 16-byte aligned, n_bytes % 16 == 0 */
    unsigned long long n_bytes;
    unsigned long long* count;   /* device */
} sfsn_count_tensor;

int sfsn_spike_count(const sfsn_count_tensor* tensors /* host */, int n_tensors, void* stream);

/* Per-clip spike counts of a streaming step run by the per-kernel sequence (the graph-replayed fallback of sfsn_stream_hop):
 * for every tensor, rows are grouped by clip (R = clips * rows_per_clip, row b * rows_per_clip + k) and
 *     counts[b] += #{ spikes_i8[t][r][c] != 0 : t0 <= t < t0 + nt, r in clip b, c < HP }
 * (pad columns are zero).  One workgroup owns each counter (plain load + store, no atomics): capturable in a HIP graph.
 * SFSN_EINVAL: NULL pointers, n_tensors outside 1 .. SFSN_MAX_COUNT_TENSORS, T, R, HP, rows_per_clip, nt <= 0, t0 < 0,
 * t0 + nt > T, R % rows_per_clip != 0, HP % 16 != 0 or a misaligned spike pointer. */
typedef struct sfsn_row_count {
    const int8_t* spikes_i8;     /* device, [T][R][HP] int8 spikes 0/1, 16-byte aligned (frame t at t * R * HP) */
    int T, R, HP, rows_per_clip;
    unsigned long long* counts;  /* device, [R / rows_per_clip], accumulated */
} sfsn_row_count;

int sfsn_spike_count_rows(const sfsn_row_count* tensors /* host */, int n_tensors, int t0, int nt, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * The two edges of the path -- replace audiozen/acoustics/audio_feature.py:236-347 as the models call them
 * (MODEL:429,473; FROZEN:568-572,612-617): torch.stft(y, n_fft, hop, n_fft, window, center=True, pad_mode="constant",
 * return_complex=True) and torch.istft(X, n_fft, hop, n_fft, window, length=length).  n_fft = 512 (every reference config;
 * SFSN_EUNSUPPORTED otherwise), n_fft % hop == 0, 4 hops per window at most.  `window` is the analysis/synthesis window on
 * the device (n_fft floats; the reference passes torch.hann_window(n_fft)).
 *   stft : frame t = samples [t*hop - n_fft/2, t*hop + n_fft/2), zero outside [0, L);  T must be 1 + L / hop
 *   istft: y[m] = sum_t w[n - t*hop] * irfft(X[:, t])[n - t*hop] / sum_t w[n - t*hop]^2,  n = m + n_fft/2,  m < length
 *          (imaginary parts of the DC and Nyquist bins are ignored, as by a complex-to-real transform)
 * ---------------------------------------------------------------------------------------------------- */
int sfsn_stft(const float* wave /* [B][L] */, int B, int L, int n_fft, int hop, const float* window,
              float* stft_ri /* [B][n_fft/2+1][T][2] */, int T, void* stream);
int sfsn_istft(const float* stft_ri /* [B][n_fft/2+1][T][2] */, int B, int T, int n_fft, int hop, const float* window,
               float* wave /* [B][length] */, int length, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * The cIRM-GSN model (CIRM = audiozen/models/cirm_gsn/modeling_cirm_gsn.py, recipes/intel_ndns/cirm_gsn): one full-band GSN stack
 * on ALL F = n_fft/2 + 1 bins and a full-spectrum deep filter.  Its GSN layers run on sfsn_gsn_stack_scan; these are its two ends
 * and its layer-0 input product.
 *
 * sfsn_fullband_features -- CIRM:220-226 + SequenceModel.forward's transpose and pre_layer_norm (CIRM:101-106):
 *     x[t][b][f] = LayerNorm_f(|X[b][f][t]|^fdrc),  f < F (Nyquist included; sfsn_features drops it)
 *     with sfsn_features' magnitude and LayerNorm expressions.  ln_w = ln_b = NULL: no LayerNorm.  F <= 320.
 *
 * sfsn_fullband_input_proj -- layer 0's input term for rows wider than sfsn_input_proj_f32 covers (K > 192: the full-spectrum rows
 * have K = F = 257): z[m][n] = sum_k x[m][k] * w[n][k] (+ bias[n]) as one fp32 fmaf chain in k order, then + bias; arguments as for
 * sfsn_input_proj_f32 (any M, K, N; ldz >= N; 4-byte aligned).
 *
 * sfsn_fullband_proj_deepfilter -- SequenceModel's proj + output activation (CIRM:113-120), the (c d s f) re-index (CIRM:230) and
 * deepfiltering (CIRM:125-157) over all F bins, in one launch:
 *     v[t][b][n] = dq'[n'] * sum_k s[t][b][k] Wq'[n'][k] + bias'[n']   (sfsn_spike_proj's arithmetic: the same value, bit for bit)
 *     C[d][s] = act(v[.][((0 * df + d) * S + s) * F + f]) + i act(v[.][((1 * df + d) * S + s) * F + f])
 *     Y[b][s][f][t] = sum_{d<df} X[b][f][t-(df-1)+d] * C[d][s]   (zero before frame 0; d ascending)
 * The projection weights are packed with their rows BIN-MAJOR: W' [NFB * NCT * 16][H] with NFB = ceil(F / 16), NCT = 2 * df * S,
 *     W'[(fb * NCT + (c * df + d) * S + s) * 16 + i] = W[((c * df + d) * S + s) * F + fb * 16 + i]   (zero rows for bins >= F)
 * and passed as sfsn_w3_pack(W', NFB * NCT * 16, H); bias' (nullable, 16-byte aligned) in the same row order.  Every row is its own
 * exact sum, so the permutation changes no bit.  `proj` (nullable) receives the pre-activation rows in the reference's column order
 * n = ((c * df + d) * S + s) * F + f, [T][B][2 * df * S * F]; they are not written anywhere when it is NULL.  enh_mag (nullable)
 * = hypot(re, im) rounded as glibc's hypotf.  Frames [t0, t0 + nt) are produced (the filter reads earlier frames of stft_ri).
 * pad64(H) <= 320, F <= 1025, S <= 4, df <= 16: SFSN_EUNSUPPORTED otherwise.  (ABI 21 additions.)
 * ---------------------------------------------------------------------------------------------------- */
#define SFSN_ACT_NONE 0    /* anything but the exact strings below: nn.Identity (CIRM:54-61) */
#define SFSN_ACT_TANH 1
#define SFSN_ACT_SIGMOID 2
#define SFSN_ACT_RELU 3

int sfsn_fullband_features(const float* stft_ri /* [B][F][T][2] */, int B, int F, int T, float fdrc, const float* ln_w /* [F] */,
                           const float* ln_b /* [F] */, float ln_eps, float* x /* [T][B][F] */, int t0, int nt, void* stream);
int sfsn_fullband_input_proj(const float* x /* [M][K] */, const float* w /* [N][K] */, const float* bias /* [N], nullable */,
                             float* z /* [M][ldz] */, int M, int K, int N, int ldz, void* stream);
int sfsn_fullband_proj_deepfilter(const float* stft_ri /* [B][F][T][2] */, const int8_t* spikes_i8 /* [T][B][pad64(H)] */, int H,
                                  const int8_t* w_packed, const float* w_dq, const float* bias, int act, int B, int F, int T, int S,
                                  int df, float* proj /* [T][B][2 df S F], nullable */, float* enh_ri /* [B][S][F][T][2] */,
                                  float* enh_mag /* [B][S][F][T], nullable */, int t0, int nt, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * The cIRM-GSN deep filter for TRAINING (training.FullbandDeepFilterFn): the coefficients are the projection's (activated) output in
 * its own layout, coef [T][B][P] with P = 2 * df * S * F and channel p = ((c * df + d) * S + s) * F + f, read / written exactly once.
 *
 * sfsn_fullband_deepfilter_fwd:
 *     Y[b][s][f][t] = sum_{d<df} X[b][f][t-(df-1)+d] * (coef[t][b][(0,d,s,f)] + i coef[t][b][(1,d,s,f)])
 *     X = 0 left of frame 0; d ascending; yr += xr * cr - xi * ci, yi += xr * ci + xi * cr (no contraction).
 * sfsn_fullband_deepfilter_bwd (the gradient with respect to coef for a cotangent g of Y; none with respect to X):
 *     d_coef[t][b][(0,d,s,f)] = xr * gr + xi * gi,  d_coef[t][b][(1,d,s,f)] = xr * gi - xi * gr,  x = X[b][f][t-(df-1)+d]
 *     Every element of d_coef is written exactly once: no zero fill is needed before the launch.
 * One workgroup = (clip, 32 frames, 32 bins): coefficient rows are read / written in runs of 32 bins (128 bytes), spectrum, output and
 * cotangent rows in runs of 32 frames (256 bytes), turned in LDS.  No atomics, no waits between workgroups, nothing per launch but the
 * launch (capturable).  B, T free; F <= 320, S <= 4, df <= 16: SFSN_EUNSUPPORTED otherwise.  spec_ri / enh_ri / g_ri 8-byte aligned.
 * (Added without an ABI bump: no struct or signature changed.)
 * ---------------------------------------------------------------------------------------------------- */
int sfsn_fullband_deepfilter_fwd(const float* spec_ri /* [B][F][T][2] */, const float* coef /* [T][B][2 df S F] */, int B, int F, int T,
                                 int S, int df, float* enh_ri /* [B][S][F][T][2] */, void* stream);
int sfsn_fullband_deepfilter_bwd(const float* spec_ri /* [B][F][T][2] */, const float* g_ri /* [B][S][F][T][2] */, int B, int F, int T,
                                 int S, int df, float* d_coef /* [T][B][2 df S F] */, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * The cIRM-GSN model frame by frame: `hop` new frames of every clip through features, GSN stack, projection and deep filter in ONE
 * launch (csrc/sfsn_fullband_hop.hip; the plan of sfsn_stream_hop: one wave per 16-neuron tile with its digits in registers, frames
 * handed from stage to stage through L2 as data-tagged granules, recurrent product before the input arrives, bounded spins with an
 * error word in scratch word 0, refused unless every workgroup can be resident).  Bit-identical to sfsn_fullband_features ->
 * sfsn_fullband_input_proj -> the GSN scans -> sfsn_fullband_proj_deepfilter on the concatenated input.
 *
 * Coverage (sfsn_fullband_hop_check, host only, no device needed; SFSN_EUNSUPPORTED outside it, SFSN_EINVAL for non-positive
 * sizes or D != df - 1):
 *     shared gate weights (unshared = 0);  Hp % 16 == 0, Hp <= 320 (hidden size padded as fullband_engine.pad_cell does);
 *     1 .. SFSN_FULLBAND_HOP_MAX_LAYERS layers;  193 <= F <= 320 (F <= 192 is sfsn_input_proj_f32's fp32-MFMA product offline);
 *     S <= 2;  df <= 5;  D + hop <= 32;  B <= 16.  BatchNorm folded into bn_alpha / bn_beta, LayerNorm optional, any SFSN_ACT_*.
 *
 * State (caller-owned, zeroed at the start of a session, touched by nothing else): per layer the last spikes h[2] [B][pad64(Hp)]
 * (double-buffered by launch parity) and the membranes c [B][Hp]; hist_ri[2] [B][F][D][2] (double-buffered likewise).  Work buffers
 * rewritten by every launch: spikes [hop][B][pad64(Hp)] per layer (tagged), z0 [hop][B][Hp][2] ({value, tag} granules of layer 0's
 * input term).  launch_index: launches made on this state so far, counted by the caller (tag and parity).  clip_start (nullable,
 * [B]): the launch index at which clip b's utterance began -- in that launch the clip's state and history read as zero.
 * Weights: w_ih0 fp32 [Hp][F] row-major; w_ih / w_hh / w_p as sfsn_w3_pack images ([Hp][Hp]; w_p bin-major as for
 * sfsn_fullband_proj_deepfilter), bias [2 Hp].  Outputs enh_ri [B][S][F][hop][2], enh_mag [B][S][F][hop] (nullable).
 * (Added without an ABI bump: no existing struct or signature changed.)
 * ---------------------------------------------------------------------------------------------------- */
#define SFSN_FULLBAND_HOP_MAX_LAYERS 4
typedef struct {
    const int8_t* w_ih;    /* layers >= 1 */
    const float* w_ih_dq;
    const int8_t* w_hh;
    const float* w_hh_dq;
    const float* bias;
    const float* bn_alpha;
    const float* bn_beta;
    int8_t* h[2];
    float* c;
    int8_t* spikes;
} sfsn_fullband_hop_layer;
typedef struct {
    sfsn_fullband_hop_layer layer[SFSN_FULLBAND_HOP_MAX_LAYERS];
    int n_layers, Hp, B, F, S, df, hop, D, act, unshared;
    float fdrc, ln_eps;
    const float* w_ih0;
    const float* ln_w; /* nullable (both): no LayerNorm */
    const float* ln_b;
    const int8_t* w_p;
    const float* w_p_dq;
    const float* b_p; /* nullable */
    const float* inp_ri; /* [B][F][hop][2] */
    float* hist_ri[2];
    float* enh_ri;
    float* enh_mag;
    float* z0;
    const unsigned* clip_start;
    void* scratch;
    size_t scratch_bytes; /* >= sfsn_fullband_hop_scratch_bytes */
    unsigned launch_index;
} sfsn_fullband_hop_desc;

int sfsn_fullband_hop_check(int Hp, int n_layers, int F, int S, int df, int B, int hop, int D, int unshared);
size_t sfsn_fullband_hop_scratch_bytes(const sfsn_fullband_hop_desc* desc); /* 0: not covered (host only) */
int sfsn_fullband_stream_hop(const sfsn_fullband_hop_desc* desc, void* stream);
/* The same launch with running spike counts (SynOPs of a streaming clip).  spike_slots: sfsn_fullband_hop_spike_slots(desc) words on the
 * device, zeroed by the caller to reset.  Layout: layer by layer; within a layer [B][Hp / 4]: slot (b, j) counts the spikes of neurons
 * 4j .. 4j + 3 of clip b (the padded neurons Hp - H never spike).  One lane of the launch owns each slot and adds, once per launch, the
 * spikes of the `hop` frames it computed (plain per-lane load + store: no atomics).  With clip_start: in the launch that restarts
 * clip b its slots read as zero instead of being loaded, as h and c do.  Everything else -- results, state, scratch, coverage -- is
 * sfsn_fullband_stream_hop's, which stays the launch of sessions that do not count (a kernel of its own).  NULL or 4-byte-misaligned
 * spike_slots: SFSN_EINVAL.  The waveform launch has no counted form.
 * (Added without an ABI bump: no existing struct or signature changed.) */
size_t sfsn_fullband_hop_spike_slots(const sfsn_fullband_hop_desc* desc); /* n_layers * B * Hp / 4; 0: not covered (host only) */
int sfsn_fullband_stream_hop_counted(const sfsn_fullband_hop_desc* desc, unsigned* spike_slots, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Waveform mode of the cIRM-GSN hop: 128 new samples per clip in, 128 enhanced samples per clip and speaker out, in ONE launch -- the
 * new frame's STFT (one workgroup in front of the input stage, a wave per clip), the hop above, and the inverse STFT with its
 * overlap-add state (ceil(B S / 8) workgroups behind the projection stage, a wave per (clip, speaker)).  The transforms are those of
 * sfsn_stft / sfsn_istft and of sfsn_hop_desc's waveform mode (csrc/sfsn_hop_wave_dev.h: one body): torch.stft(center=True,
 * pad_mode="constant") framing, torch.istft's overlap-add and envelope, bit-identical to the offline kernels.
 *
 * Coverage (sfsn_fullband_wave_hop_check, host only, no device needed): what sfsn_fullband_hop_check returns at hop = 1, D = df - 1,
 * and SFSN_EUNSUPPORTED unless F == 257 (512-point frames with hop 128 are what csrc/sfsn_fft_dev.h implements).
 *
 * The descriptor embeds the hop's: hop.hop == 1, hop.D == hop.df - 1 (SFSN_EINVAL otherwise); hop.inp_ri is ignored; hop.enh_ri and
 * hop.enh_mag are nullable (written when set); hop.clip_start is REQUIRED -- the frame index of every clip comes from it.  With
 * k = (int)(hop.launch_index - hop.clip_start[b]) (unsigned difference, wrap-safe):
 *     k == -1   the clip's first call, no frame yet: its old wave_state reads as zero and the launch leaves [0 x 384 | the new samples]
 *               in it; whatever the model stages write for the clip is discarded by the next launch
 *     k ==  0   the clip's frame 0: h, c, the history and ola_state read as zero; wave_state is loaded
 *     k  <  2   wave_out of clip b is zero
 *     k >=  2   wave_out holds the padded positions [128 k, 128 k + 128): call c of an utterance returns the samples that entered
 *               with call c - 3
 * So a session starts with clip_start[b] = launch_index + 1, and restarts a clip by writing (stream-ordered) the index of the launch
 * after the next one.  Every granule of spec_g and enh_g is written by every launch for every clip, whatever its k.
 * NULL or misaligned (8 bytes; done: 4) required pointers: SFSN_EINVAL.  Scratch and the error word: as for sfsn_fullband_stream_hop
 * (sfsn_fullband_hop_scratch_bytes(&desc->hop)).  The launch is refused (SFSN_EUNSUPPORTED) unless all its workgroups -- at most
 * 1 + 4 more than the spectrum hop's -- can be resident.
 * (Added without an ABI bump: no existing struct or signature changed.)
 * ---------------------------------------------------------------------------------------------------- */
typedef struct {
    sfsn_fullband_hop_desc hop;
    const float* wave_in; /* [B][128] the new samples                                                         */
    float* wave_state;    /* [B][512] the last 512 input samples, in/out                                       */
    float* ola_state;     /* [B][S][512] overlap-add accumulator of the output, in/out                         */
    float* wave_out;      /* [B][S][128] out                                                                   */
    const float* window;  /* [512] analysis / synthesis window (the reference: hann)                           */
    float* spec_g;        /* [B][F][4] scratch ({re, tag, im, tag} granules of the noisy frame), zeroed once     */
    float* enh_g;         /* [B][S][F][4] scratch (granules of the enhanced frame), zeroed once                 */
    unsigned* done;       /* nullable, [B][S]: word (b, s) is set to launch_index + 1 (system-scope release) once wave_out (b, s)
                             has been written.  wave_in, wave_out and done may be pinned host memory the device can reach: the
                             caller spins on the words instead of synchronising the stream                       */
} sfsn_fullband_wave_desc;

int sfsn_fullband_wave_hop_check(int Hp, int n_layers, int F, int S, int df, int B, int unshared);
int sfsn_fullband_stream_hop_wave(const sfsn_fullband_wave_desc* desc, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * The cIRM-GSN hop with HELD clips: bit b of held_mask = clip b has no frame (no samples) this tick and sits launch
 * k = desc->launch_index out.  ONE launch and nothing else on the stream: B <= 16 for this kernel, so the mask is one word by value in
 * the kernel arguments -- no device buffer exists that a queued launch could find overwritten, and no copy is enqueued.
 * held_mask == 0 IS the existing launch: sfsn_fullband_stream_hop (spike_slots == NULL), sfsn_fullband_stream_hop_counted or
 * sfsn_fullband_stream_hop_wave, the same kernels, which do not carry the mask (the held forms are three kernels of their own: held,
 * held + counted, held waveform).
 *
 * Every stage, hand-off, granule and tag runs for every row as in the plain launch.  Rows are independent in the LayerNorm, the
 * layer-0 fmaf chains, the MFMA products (a clip is a column) and the deep filter, so a held clip's rows compute on whatever inp_ri /
 * wave_in hold for them (anything, NaN included; nothing of it reaches another clip or any carried state) and no wait is added.  For a
 * held clip b in launch k:
 *   h                      h[(k + 1) & 1] row <- the bytes of h[k & 1] row, instead of the last frame's spikes
 *   c                      not written
 *   spike_slots            not added to, nor zeroed
 *   layer.spikes           (work buffer) published with its tag as always: every tile gathers all rows
 *   hist_ri                hist_ri[(k + 1) & 1] rows <- hist_ri[k & 1] rows, no shift, none of the new frames.  (The sibling's history is
 *                          one buffer and simply stays; this one is double-buffered by launch parity, so it must cross.)  Written by
 *                          the speaker-0 workgroups only, as always; with D == 0 nothing is written
 *   enh_ri, enh_mag        written as zero for all S speakers and all `hop` frames
 *   enh_g granules         leave (zeros) with their tag: the inverse-STFT waves poll them
 *   wave_state             not shifted; a first call (k == clip_start[b] - 1) does not take the samples
 *   ola_state              not touched
 *   wave_out               zero
 *   done                   written as always (launch_index + 1): a host that spins on the words returns
 *   clip_start[b] += 1     (unsigned): the clip's origin moves on by one launch, so that launch k + 1 -- and
 *                          sfsn_fullband_hop_state_export / _import and sfsn_fullband_hop_seed / _advance, which all read clip b
 *                          through its origin -- see it exactly as if launch k had never happened for it: a restart or first call
 *                          that was due in launch k is due in k + 1
 * The origin rule (sfsn_stream_hop_held's): the + 1 is ordered after every read of clip_start in this launch and before the next launch
 * on the stream.  Each workgroup, its role done and nothing of it in flight, adds 1 (vector atomic) to word 3 of `scratch` as its last
 * act -- also a workgroup whose bounded wait expired, and the inverse-STFT waves that have no pair -- and the workgroup that finds
 * itself last applies the + 1s and clears the word.  Nobody waits on that word: no spin is added.  Word 0 stays the error word, words
 * 1 and 2 are unused, sfsn_fullband_hop_scratch_bytes stays 64.  clip_start must therefore be device-writable memory the caller hands
 * over for the launch; the caller still numbers the launches itself (launch_index + 1 after this one too) and does not advance its own
 * count of a held clip's frames / calls.
 *
 * Returns, with held_mask == 0, what the plain launch returns.  With a bit set, in this order -- the mask checks come before any
 * device query, so they are answered without a device:
 *   desc == NULL                                        SFSN_EINVAL
 *   a bit at or beyond desc->B                          SFSN_EINVAL
 *   desc->clip_start == NULL                            SFSN_EINVAL   (a held clip needs an origin of its own)
 *   a descriptor the plain launch refuses               the plain launch's code
 *   spike_slots misaligned (4 bytes)                    SFSN_EINVAL
 * spike_slots == NULL: the uncounted launch.  (Added without an ABI bump: no existing struct or signature changed.)
 * ---------------------------------------------------------------------------------------------------- */
int sfsn_fullband_stream_hop_held(const sfsn_fullband_hop_desc* desc, unsigned* spike_slots /* nullable: the uncounted launch */,
                                  unsigned held_mask /* bit b = clip b sits launch desc->launch_index out */, void* stream);
int sfsn_fullband_stream_hop_wave_held(const sfsn_fullband_wave_desc* desc, unsigned held_mask, void* stream);

/* sfsn_fullband_stream_hop_wave / _wave_held for OUTER samples that differ from the model's (sfsn_hop_io, as it stands above
 * sfsn_stream_hop_io: three times the model's rate and / or 16-bit PCM): the conversion runs in the launch's first and last role, by the
 * waves that build the frame and that finish the inverse STFT -- no further launch, wait, hand-off, tag or workgroup
 * (csrc/sfsn_fullband_hop_io.hip; the device bodies are sfsn_stream_hop_io's, csrc/sfsn_hop_wave_dev.h).
 * io == NULL IS sfsn_fullband_stream_hop_wave_held(desc, held_mask, stream) (and with held_mask == 0, sfsn_fullband_stream_hop_wave).
 * Otherwise desc->wave_in and desc->wave_out are ignored and, with k = (int)(hop.launch_index - hop.clip_start[b]), the launch
 *   reads   io->wave_in [B][128 ratio] (8-byte aligned, as wave_in is); every clip's dec_state row (as zero in the clip's first call,
 *           k == -1, which is how a restart reaches the filter with no extra launch); every pair's int_state row; taps, phase_taps; all
 *           sfsn_fullband_stream_hop_wave reads;
 *   writes  io->wave_out [B][S][128 ratio] (8-byte aligned): U3(the 128 samples sfsn_fullband_stream_hop_wave would have written) in
 *           io->format, stored before the pair's done word; ZERO while k < 2, and int_state is then written as zero: the interpolator
 *           sees the zeros its caller sees;
 *           wave_state [B][512]: the last 512 samples at the MODEL's rate, D3(io->wave_in) appended; dec_state: the last 93 outer samples;
 *           everything else sfsn_fullband_stream_hop_wave writes.
 *   held    (bit b of held_mask) as sfsn_fullband_stream_hop_wave_held, and: dec_state and int_state of the clip are not touched,
 *           io->wave_out of the clip is zero in io->format.
 * ratio 1 with SFSN_SAMPLE_F32 launches the kernels of sfsn_fullband_stream_hop_wave(_held) on io's buffers; the other three
 * combinations have instantiations of their own (held and not), in which the plain kernels' code is unchanged.  The launch's dynamic
 * LDS is the plain launch's or, with ratio 3, at least the STFT role's 40 KB with the decimator windows; the 160 KB refusal stays.
 * Returns, in this order:
 *   io->ratio not 1 or 3                                                   SFSN_EINVAL
 *   io->format unknown                                                     SFSN_EINVAL
 *   desc NULL or desc->wave_state NULL                                     SFSN_EINVAL
 *   a NULL io->wave_in / wave_out; ratio 3: a NULL state or tap pointer    SFSN_EINVAL
 *   with a bit of held_mask set: sfsn_fullband_stream_hop_held's mask checks (a bit at or beyond B, clip_start NULL: SFSN_EINVAL)
 * then whatever sfsn_fullband_stream_hop_wave returns.  The refusals listed are answered without a device.
 * (Added without an ABI bump: no existing struct or signature changed.) */
int sfsn_fullband_stream_hop_wave_io(const sfsn_fullband_wave_desc* desc /* host */, const sfsn_hop_io* io /* host, nullable */,
                                     unsigned held_mask, void* stream);

/* Moving a clip of a cIRM-GSN session (csrc/sfsn_state.hip): sfsn_hop_state_export / sfsn_hop_state_import for sfsn_fullband_hop_desc --
 * the same launch, the same rules (one launch, plain stores, the half of h and hist_ri that launch launch_index reads, scratch and z0
 * untouched, the origin kept by the caller: clip_start[b'] = launch_index - age) and the same return codes.  What lives outside the
 * descriptor is handed over as the launches take it: spike_slots as sfsn_fullband_stream_hop_counted does (NULL: the session does not
 * count), wave_state and ola_state of a sfsn_fullband_wave_desc whose `hop` is `desc` (both NULL: a spectrum session; one NULL:
 * SFSN_EINVAL; with spike_slots: SFSN_EUNSUPPORTED, the waveform launch has no counted form).
 *
 * Blob of sfsn_fullband_hop_state_export: one clip = sfsn_fullband_hop_state_bytes(desc, counted, wave) bytes.  Sections in this order,
 * each starting at the next multiple of 16 bytes, the total rounded up to a multiple of 16:
 *   for every layer:   h int8 [Hp] the last frame's spike bytes,  c float [Hp] the membranes
 *   slots  u32   [Hp / 4]      only if counted: for every layer
 *   hist   float [F][D][2]     only if D > 0: the last D noisy frames
 *   wave   float [512]         only in waveform mode: wave_state
 *   ola    float [S][512]      only in waveform mode: ola_state
 * sfsn_fullband_hop_state_bytes is host only; 0: outside sfsn_fullband_hop_check (wave: sfsn_fullband_wave_hop_check), or counted with wave.
 * (Added without an ABI bump: no existing struct or signature changed.) */
size_t sfsn_fullband_hop_state_bytes(const sfsn_fullband_hop_desc* desc, int counted, int wave);
int sfsn_fullband_hop_state_export(const sfsn_fullband_hop_desc* desc, const unsigned* spike_slots /* nullable */,
                                   const float* wave_state /* nullable */, const float* ola_state /* nullable */, const int* clips /* host */,
                                   int n_clips, void* blob /* device [n_clips][bytes] */, void* stream);
int sfsn_fullband_hop_state_import(const sfsn_fullband_hop_desc* desc, unsigned* spike_slots /* nullable */, float* wave_state /* nullable */,
                                   float* ola_state /* nullable */, const int* clips /* host */, int n_clips,
                                   const void* blob /* device [..][bytes] */, int b0 /* first blob row */, void* stream);

/* A backlog on a RUNNING clip of a cIRM-GSN session (csrc/sfsn_prime.hip): sfsn_hop_seed / sfsn_hop_advance for sfsn_fullband_hop_desc --
 * the same two kernels from host-filled params (one sequence, one row per clip, H = Hp), the same rules: N new frames go through the
 * OFFLINE kernels (sfsn_fullband_features -> sfsn_fullband_input_proj -> the GSN scans -> sfsn_fullband_proj_deepfilter), started from
 * the state the session carries, and their end state is handed back.  One launch each, for the listed clips only (distinct indices,
 * 1 <= n_clips <= B <= 16); every other clip's rows, scratch, z0, the tagged spikes buffers and launch_index are left as they are.
 * Plain loads and stores, no atomics, nothing waits; ordered on `stream` like any launch.  k = desc->launch_index.  What lives
 * outside the descriptor is handed over as for the state launches above: spike_slots (NULL: the session does not count), wave_state
 * and ola_state of the sfsn_fullband_wave_desc whose `hop` is `desc` (waveform mode: wave_state != NULL).
 *
 * sfsn_fullband_hop_seed: the offline kernels' START tensors, rows b0 + i of tensors of Bp clips for clips[i]:
 *   layer.h   <- h[k & 1] as fp32 0 / 1 [Bp][Hp] (the hop's row stride is pad64(Hp)), layer.c <- c;
 *   stft_ri   <- frames [0, D) of every row [F][T][2] = hist_ri[k & 1], the half of the double buffer that launch k reads.  The
 *                caller puts the N new frames at [T - N, T), T >= D + N, and runs the offline stages on those frames of the buffer;
 *   wave_ctx  <- waveform mode: wave_state[128 .. 512) at the front of a row of wave_stride floats (the caller appends the new
 *                samples: frame j of the backlog is the centred frame j + 2 of that row on sfsn_stft).
 * desc->clip_start is read (required in waveform mode): a clip whose origin equals k (restarted or never stepped: the hop reads its
 * state as zero in launch k, whatever memory holds) is written as zeros everywhere but wave_ctx.  Waveform mode: a clip whose origin
 * equals k + 1 (no call yet: launch k is its first call, which has no frame and reads the old samples as zero) is written as zeros,
 * wave_ctx included -- so [0 x 384 | its samples] holds its first call's STFT state, and its frame j is the centred frame j + 3.
 *
 * sfsn_fullband_hop_advance: `src` holds the offline kernels' results for the N new frames.
 *   layer.h[k & 1], layer.c <- frame N - 1 of spikes_i8, and c (the end state of the backlog);
 *   hist_ri[k & 1] <- the last D frames of stft_ri's rows of T frames, [history | new]: N < D keeps the tail of the old history;
 *   spike_slots  <- ADDED to: slot (b, j) += the spikes of neurons 4j .. 4j + 3 over the N frames (a clip whose origin equals k:
 *                   replaced, the hop reads its slot as zero);
 *   wave_state   <- wave_tail, the last 512 input samples; ola_state <- continued in the hop's order: the carried partial sums first
 *                   (zero for a clip whose origin equals k or k + 1), then frames T - N .. T - 1 of enh_ri's rows in ascending order
 *                   (sfsn_hop_wave_dev.h's arithmetic and envelope); wave_out[b0 + i][s][128 j ..] <- the block the launch that
 *                   computes the clip's new frame j would have written (zero while that frame's index is < 2).  For a clip that
 *                   has made a call that is launch k + j; for a clip without a call launch k + 1 + j (launch k, its first call,
 *                   writes a block of zeros, which the caller puts in front).
 * N = 0 is legal in waveform mode only -- the clip without a call and one call's worth of samples: wave_state <- wave_tail, and h, c,
 * hist_ri, ola_state are written as zero (which its frame 0 reads whatever memory holds).
 * The caller then moves clip_start[clips[i]] back by the launches replaced -- N / hop; waveform mode: the calls replaced, N for a
 * clip that had made a call, N + 1 for a clip that had not -- unsigned, wrap-safe, with a stream-ordered device operation behind the
 * queued launches.
 *
 * Exactness: bit for bit what the launches would have left, layer 0 included -- sfsn_fullband_stream_hop is bit-identical to the
 * offline sequence (above), so this pair carries no layer-0 reservation (sfsn_hop_advance has one).
 * SFSN_EINVAL, before any launch: a NULL desc / clips / dst / src, n_clips < 1, an index outside [0, desc->B) or listed twice,
 * b0 + n_clips > Bp, N % hop != 0, N < hop (waveform mode: N < 0), T < D + N (seed: T < D), wave_stride < 384, one of wave_state /
 * ola_state NULL, a missing or misaligned pointer (h, c: 16 bytes; stft_ri, enh_ri, wave_out, ola_state: 8; the others: 4).
 * SFSN_EUNSUPPORTED: a descriptor sfsn_fullband_hop_check (waveform mode: sfsn_fullband_wave_hop_check) refuses, spike_slots together
 * with wave_state (the waveform launch has no counted form).  (Added without an ABI bump: no existing struct or signature changed.) */
typedef struct sfsn_fullband_seed_dst {
    int Bp, T, b0;
    int wave_stride;         /* waveform mode: floats per row of wave_ctx (>= 384)                   */
    float* stft_ri;          /* [Bp][F][T][2]: frames [0, D) are written (NULL if D == 0)            */
    float* wave_ctx;         /* waveform mode: [Bp][wave_stride], samples [0, 384) are written       */
    sfsn_seed_layer layer[SFSN_FULLBAND_HOP_MAX_LAYERS]; /* h, c: [Bp][Hp]                           */
} sfsn_fullband_seed_dst;
typedef struct sfsn_fullband_advance_src {
    int Bp, N, b0;
    int T;                   /* frames per row of stft_ri / enh_ri; the N new frames are the last ones  */
    const float* stft_ri;    /* [Bp][F][T][2] [history | new] (NULL if D == 0 or N == 0)                */
    const float* enh_ri;     /* waveform mode: [Bp][S][F][T][2] the enhanced frames (NULL if N == 0)    */
    const float* wave_tail;  /* waveform mode: [Bp][512] the last 512 input samples                     */
    float* wave_out;         /* waveform mode: [Bp][S][128 * N] out (NULL if N == 0)                    */
    const float* window;     /* waveform mode: [512] the session's window (sfsn_fullband_wave_desc)     */
    sfsn_prime_layer layer[SFSN_FULLBAND_HOP_MAX_LAYERS]; /* spikes_i8: the N new frames' [N][Bp][pad64(Hp)]; c [Bp][Hp]: after the last */
} sfsn_fullband_advance_src;
int sfsn_fullband_hop_seed(const sfsn_fullband_hop_desc* desc /* host */, const unsigned* spike_slots /* nullable */,
                           const float* wave_state /* nullable */, const int* clips /* host */, int n_clips,
                           const sfsn_fullband_seed_dst* dst /* host */, void* stream);
int sfsn_fullband_hop_advance(const sfsn_fullband_hop_desc* desc /* host */, unsigned* spike_slots /* nullable */,
                              float* wave_state /* nullable */, float* ola_state /* nullable */, const int* clips /* host */, int n_clips,
                              const sfsn_fullband_advance_src* src /* host */, void* stream);

/* sfsn_fullband_hop_advance with a backlog of ITS OWN LENGTH per clip (csrc/sfsn_prime.hip; a kernel of its own): sfsn_hop_advance_ragged's
 * contract on sfsn_fullband_hop_advance's state.  The offline kernels ran ONE padded forward of Nmax new frames behind T - Nmax >= D
 * frames of history (the padding zeroed; sfsn_fullband_proj_deepfilter_ragged as the epilogue, the per-layer scans with the membrane
 * tap), clip b0 + i has N_b = frames[b0 + i] of them (device int32 [Bp], each a multiple of hop with hop <= N_b <= Nmax: the CALLER's
 * check -- the launch holds a value outside [1, Nmax] inside that range, so that no index leaves the tensors, and promises nothing else
 * about such a clip).  For clips[i], with k = desc->launch_index:
 *   layer.h[k & 1] <- row N_b - 1 of spikes_i8; layer.c <- row N_b - 1 of `membrane` (sfsn_scan_segment.membrane: c_state itself is the
 *                     membrane after the last PADDED frame and is not read);
 *   hist_ri[k & 1] <- the D frames that end with frame T - Nmax + N_b - 1 of stft_ri's row: N_b < D keeps the tail of the old history;
 *   spike_slots    <- ADDED to over frames [0, N_b) only (a clip whose origin equals k: replaced);
 *   wave_state     <- the 512 samples that end at sample 384 + 128 N_b of the clip's row of wave_ctx ([384 of context | new samples],
 *                     the row sfsn_fullband_hop_seed began); ola_state <- continued in the hop's order through frame N_b - 1 only;
 *                     wave_out[b0 + i][s][128 j ..] <- block j < N_b as sfsn_fullband_hop_advance writes it, zeros for N_b <= j < Nmax.
 * Waveform mode, a clip WITHOUT A CALL (origin k + 1; the launch reads desc->clip_start): it carries no overlap-add sums, its first
 * new frame has frame index 0, its N_b may be 0 (held inside [0, Nmax]; its backlog is its first call alone: zeros to h, c, hist_ri
 * and ola_state, only wave_state taken) and its window of samples ends ONE HOP LATER, at sample 384 + 128 (N_b + 1) of its row -- its
 * first 128 samples made no frame.  Rows of such clips hold wave_stride >= 384 + 128 (Nmax + 1) floats; the host cannot know a clip's
 * kind, so the launch holds the window's end inside the row.
 * The caller then moves clip_start[clips[i]] back by the clip's OWN launches replaced -- N_b / hop; waveform mode: N_b calls for a clip
 * that had made a call, N_b + 1 for one that had not -- unsigned, wrap-safe, stream-ordered, behind the queued launches.  Everything
 * else -- the untouched clips and scratch, exactness without a layer-0 reservation -- is sfsn_fullband_hop_advance's.  Plain vector
 * loads and stores, no atomics, nothing waits.
 * SFSN_EINVAL, before any launch: as sfsn_fullband_hop_advance with Nmax in the place of N (Nmax % hop != 0, Nmax < hop in either mode,
 * T < D + Nmax), a missing or misaligned pointer (membrane: 16 bytes; stft_ri, enh_ri, wave_out: 8; frames, spikes_i8, wave_ctx,
 * window: 4), wave_stride < 384 + 128 Nmax.  SFSN_EUNSUPPORTED: as sfsn_fullband_hop_advance.  (Added without an ABI bump: a new
 * function and a new struct only.) */
typedef struct sfsn_fullband_advance_ragged_src {
    int Bp, Nmax, b0;
    int T;                   /* frames per row of stft_ri / enh_ri; the Nmax (padded) new frames are the last ones */
    int wave_stride;         /* waveform mode: floats per row of wave_ctx (>= 384 + 128 Nmax; see above)            */
    const int* frames;       /* DEVICE int32 [Bp]: N_b, the new frames clip b0 + i really has                      */
    const float* stft_ri;    /* [Bp][F][T][2] [history | new | padding] (NULL if D == 0)                           */
    const float* enh_ri;     /* waveform mode: [Bp][S][F][T][2] the enhanced frames                                */
    const float* wave_ctx;   /* waveform mode: [Bp][wave_stride] 384 samples of context, then the new samples      */
    float* wave_out;         /* waveform mode: [Bp][S][128 * Nmax] out                                             */
    const float* window;     /* waveform mode: [512] the session's window (sfsn_fullband_wave_desc)                */
    sfsn_ragged_layer layer[SFSN_FULLBAND_HOP_MAX_LAYERS]; /* spikes_i8 [Nmax][Bp][pad64(Hp)], membrane [Nmax][Bp][Hp] */
} sfsn_fullband_advance_ragged_src;
int sfsn_fullband_hop_advance_ragged(const sfsn_fullband_hop_desc* desc /* host */, unsigned* spike_slots /* nullable */,
                                     float* wave_state /* nullable */, float* ola_state /* nullable */, const int* clips /* host */,
                                     int n_clips, const sfsn_fullband_advance_ragged_src* src /* host */, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * The intel_ndns recipe's training loss (recipes/intel_ndns/spiking_fullsubnet/trainer.py:24-48 on audiozen/loss.py) and its
 * gradient with respect to the estimate, in one call of two launches:
 *     freq  = mean |Re E - Re T| + mean |Im E - Im T|          (freq_MAE, loss.py:138-155)
 *     mag   = mean | |E| - |T| |                               (mag_MAE, loss.py:167-183)
 *     sisnr = mean over rows of 10 log10(ratio + eps)          (SISNRLoss, loss.py:25-40; eps = 2^-23)
 *     total = c_freq freq + c_mag mag + c_sdr sisnr
 * E, T = torch.stft(x, 2048, 512, window=hann_window(2048), center=True, pad_mode="reflect", return_complex=True) of est, tgt
 * [rows][n_samples]: T' = 1 + n_samples / 512 frames per row, bins 0..1024, means over rows * 1025 * T' elements.  SI-SNR per row:
 * both signals minus their means, proj = <s_t, s_e> s_t / |s_t|^2, ratio = |proj|^2 / (|s_e - proj|^2 + eps); an all-zero target
 * row gives what IEEE arithmetic gives.
 *   flags     SFSN_LOSS_* bits: the terms that are computed; the others are reported as 0 and take no part in total or gradient
 *             (SDR alone runs no transform)
 *   terms     [4] device, 16-byte aligned: freq, mag, sisnr, total
 *   grad_est  [rows][n_samples] device, d total / d est (sgn(0) = 0 and E / |E| = 0 at E = 0, ATen's conventions); NULL: forward only
 *   scratch   the scratch-bytes function's size, 16-byte aligned; needs no initialisation and carries nothing between calls
 * Deterministic: no atomics, every sum in a fixed order; repeated calls and graph replays return the same bits.  Capturable: no host
 * synchronisation, no waits between workgroups.
 * Checked before any launch: NULL or misaligned pointer, rows < 1, flags outside 1..7, n_samples <= 1024 (the reflect padding of
 * 1024 samples is undefined there; torch.stft raises) -> SFSN_EINVAL; rows * n_samples or rows * T' * 2048 >= 2^31 ->
 * SFSN_EUNSUPPORTED.  The scratch-bytes function returns 0 for a shape the call refuses.
 * ---------------------------------------------------------------------------------------------------- */
#define SFSN_LOSS_FREQ 1
#define SFSN_LOSS_MAG 2
#define SFSN_LOSS_SDR 4
size_t sfsn_recipe_loss_scratch_bytes(int rows, int n_samples);
int sfsn_recipe_loss(const float* est /* [rows][n_samples] */, const float* tgt /* [rows][n_samples] */, int rows, int n_samples,
                     float c_freq, float c_mag, float c_sdr, int flags, float* terms /* [4] */, float* grad_est /* nullable */,
                     void* scratch, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * The recipe loss on rows of different lengths in one padded batch, with the REVERB recipe's time-domain L1 as a fourth term
 * (recipes/reverb/spiking_fullsubnet/trainer.py:34-37: freq_MAE + mag_MAE + F.l1_loss(est_y, ref_y)).  est, tgt [rows][n_samples],
 * n_samples the padded row stride.  Row r has L_r = row_len[r] samples, clamped on the device into [1025, n_samples] so that a wrong
 * value never indexes outside the row; T_r = 1 + L_r / 512 frames and N_r = 1025 T_r spectral terms.
 * Every row term is what sfsn_recipe_loss returns for the row alone (rows = 1, n_samples = L_r), with the bits of that call:
 *     freq_r, mag_r   reflect padding about the row's own samples 0 and L_r - 1, means over N_r
 *     sisnr_r         10 log10(ratio + eps) over the row's L_r samples (means and eps as above)
 *     time_r          sum |e - t| / L_r, summed in fp64
 * A batch term is the mean of the fp32 row terms, every row weighted equally whatever its length, accumulated in fp64 in row order:
 *     freq = (1 / rows) sum_r freq_r, likewise mag, sisnr, time;  total = ((c_freq freq + c_mag mag) + c_sdr sisnr) + c_time time
 * With equal lengths every N_r is the same and this is the reference's mean over the batch.
 *   row_len   [rows] device int32, 16-byte aligned at its base; NULL: every row has n_samples
 *   flags     SFSN_LOSS_* bits, 1..15; a term whose bit is clear is reported as 0 and takes no part in total or gradient (SDR and
 *             TIME, alone or together, run no transform)
 *   terms     [5] device: freq, mag, sisnr, time, total
 *   row_terms [rows][4] device or NULL: freq_r, mag_r, sisnr_r, time_r
 *   grad_est  [rows][n_samples] device or NULL (forward only, the same values): d total / d est.  Row r's share carries the factor
 *             1 / rows: its spectral coefficients are (float)(c / (rows N_r)), its SI-SNR term has c_sdr / rows, and the time term
 *             (float)(c_time sgn(e - t) / (rows L_r)), sgn(0) = 0, is added to a sample after the SI-SNR term.  Samples at and beyond
 *             L_r are written as exactly 0.0f.
 *   scratch   the scratch-bytes function's size, 16-byte aligned; needs no initialisation and carries nothing between calls
 * Nothing at or beyond L_r is read, in est or in tgt: the padding may hold anything, NaN included.
 * Deterministic and capturable like sfsn_recipe_loss: two plain launches sized on the padded row, no atomics, no waits between
 * workgroups, no host synchronisation; the lengths are read on the device.
 * Checked before any launch: NULL est, tgt, terms or scratch, a misaligned pointer, rows < 1, flags outside 1..15, n_samples <= 1024
 * -> SFSN_EINVAL; rows * n_samples or rows * T' * 2048 >= 2^31 (T' of the padded row) -> SFSN_EUNSUPPORTED.  The scratch-bytes
 * function returns 0 for a shape the call refuses.  (Added without an ABI bump: no existing struct or signature changed.)
 * ---------------------------------------------------------------------------------------------------- */
#define SFSN_LOSS_TIME 8
size_t sfsn_recipe_loss_ragged_scratch_bytes(int rows, int n_samples);
int sfsn_recipe_loss_ragged(const float* est /* [rows][n_samples] */, const float* tgt /* [rows][n_samples] */, int rows, int n_samples,
                            const int32_t* row_len /* nullable [rows] */, float c_freq, float c_mag, float c_sdr, float c_time, int flags,
                            float* terms /* [5] */, float* row_terms /* nullable [rows][4] */, float* grad_est /* nullable */,
                            void* scratch, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * The wsj0-mix recipes' training loss, PITWrapper(PairwiseNegSDR()) of audiozen/pit.py (recipes/wsj0-mix/spiking_fullsubnet/
 * trainer.py:24-33), and its gradient with respect to the estimates, in one call of two launches.  est, ref [clips][sources][n_samples].
 * For clip b, estimate i and reference j (pit.py:11-56), with a = est[b][i] and r = ref[b][j], each minus its own mean when zero_mean:
 *     dot = <a, r>,  tn = |r|^2,  alpha = dot / (tn + eps),  proj = alpha r,  noise = a - proj
 *     pair[b][i][j] = -10 log10(|proj|^2 / (|noise|^2 + eps) + eps)
 * Permutations p of 0..S-1 in the order of itertools.permutations (pit.py:63-94):
 *     loss_p[b] = (1 / S) sum_j pair[b][p[j]][j];  perm[b] = the p with the smallest loss_p[b], on an exact tie the earliest in that order
 *     loss = mean_b min_p loss_p[b];  reordered[b][j] = est[b][perm[b][j]] (the input's own bits)
 * The sums behind pair are accumulated in fp64 and |noise|^2 = |a|^2 - 2 alpha dot + alpha^2 tn is formed from them in fp64; pair is
 * rounded to fp32 once, and the search adds those fp32 values (in fp64, j ascending), so perm is the first minimum of the pair the
 * caller reads.
 *   pair_cot  NULL: PIT mode.  pair, perm [clips][sources] and loss [1] are written; grad_est = d loss / d est, i.e. 1 / (clips S)
 *             times d pair[b][perm[b][j]][j] / d est on row perm[b][j], through the mean subtraction when zero_mean; reordered
 *             (nullable) as above.
 *             [clips][S][S]: pairwise mode.  perm, loss and reordered must be NULL; pair is written;
 *             grad_est[b][i] = sum_j pair_cot[b][i][j] d pair[b][i][j] / d est[b][i].
 *   grad_est  [clips][sources][n_samples] or NULL: forward only, with the same values.  It is written as A est + sum_j R_j ref_j + C per
 *             row with fp32 coefficients A, R_j, C (d pair / d a = ca a + cr r with
 *             ca = (20 / ln 10) P / (arg den^2), cr = -(20 / ln 10) alpha / arg (tn / (tn' den) + P (1 + eps / tn') / den^2),
 *             P = alpha^2 tn, den = |noise|^2 + eps, arg = P / den + eps, tn' = tn + eps; the means leave the constant C)
 *   scratch   the scratch-bytes function's size, 16-byte aligned; needs no initialisation and carries nothing between calls
 * Every pointer is device memory; est, ref, pair_cot, pair, perm, loss, grad_est, reordered and scratch are 16-byte aligned at their
 * base (rows inside need not be: n_samples % 4 != 0 is covered).
 * Deterministic: no atomics, every sum in a fixed order; repeated calls and graph replays return the same bits.  Capturable: two plain
 * launches on the caller's stream, no host synchronisation, no waits between workgroups.
 * Checked before any launch: a NULL est, ref, pair, scratch, or (PIT mode) perm or loss; a base pointer that is not 16-byte aligned;
 * clips < 1, sources < 1 or n_samples < 2; eps negative or not finite; perm, loss or reordered given together with pair_cot
 * -> SFSN_EINVAL.  sources > 4, or clips * sources * n_samples >= 2^31 -> SFSN_EUNSUPPORTED.  The scratch-bytes function returns 0
 * exactly for the shapes the call refuses.
 * ---------------------------------------------------------------------------------------------------- */
size_t sfsn_pit_sdr_scratch_bytes(int clips, int sources, int n_samples);
int sfsn_pit_sdr(const float* est, const float* ref /* [clips][sources][n_samples] */, int clips, int sources, int n_samples, int zero_mean,
                 float eps, const float* pair_cot /* nullable [clips][S][S] */, float* pair /* [clips][S][S] */,
                 int32_t* perm /* [clips][S] */, float* loss /* [1] */, float* grad_est /* nullable */, float* reordered /* nullable */,
                 void* scratch, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Ragged batches: clips of different lengths, zero-padded into one batch (csrc/sfsn_ragged.hip).  Everything of a forward that
 * depends on where a clip ends sits at the edges of the path -- STFT, inverse STFT, the utterance statistics of the frozen
 * front-end, spike counts -- and each of those calls has a sibling here that takes the clips' own lengths: device int32 arrays
 * with one entry per clip, `clip_len` [B] in samples and `clip_frames` [B] in frames (T_b = 1 + L_b / hop).  The scans need none:
 * the model is causal, frames t < T_b of a padded clip are those of the clip alone.
 *
 * Contract: clip b of a ragged call has, over its valid range, the BITS of the equal-length call on that clip alone (B = 1,
 * T = T_b, L = length = L_b): the same expressions on the same values in the same order; what the padding would contribute is
 * skipped, never added as +0 and never reordered.  The lengths are read on the device (no host synchronisation) and clamped
 * to the buffer's extent before any address is formed; what the host can check it checks before any launch: NULL pointers (the
 * length arrays included), B <= 0 (B > 65535 where B is a grid dimension) and the sibling's own conditions -> SFSN_EINVAL,
 * n_fft != 512 -> SFSN_EUNSUPPORTED.  All are capturable in a HIP graph.
 *
 *   sfsn_stft_ragged            sfsn_stft; samples at index >= clip_len[b] read as zero whatever the buffer holds.  All T frames are
 *                               written (frames t >= T_b: the transform of what remains of the clip, then of zeros).
 *   sfsn_istft_ragged           sfsn_istft; frames t >= clip_frames[b] do not exist for clip b (they add nothing to the overlap-add
 *                               sum and nothing to the window envelope, whatever stft_ri holds there); samples m >= clip_len[b] are
 *                               written as 0.  Tile origin, ascending-frame accumulation and the env > 1e-11f rule are sfsn_istft's.
 *   sfsn_laplace_means_ragged   sfsn_laplace_means / sfsn_gaussian_stats; the row sums run over t < clip_frames[b], the divisor
 *   sfsn_gaussian_stats_ragged  (Gaussian: n and n - 1) uses the clip's own T_b.  Same scratch sizes.  Gaussian: clip_frames[b] >= 2
 *                               is the caller's to ensure (T < 2 -> SFSN_EINVAL).
 *   sfsn_spike_count_rows_ragged  sfsn_spike_count_rows for B clips per tensor (R == B * rows_per_clip, else SFSN_EINVAL):
 *                               counts[b] += #{ spikes : t0 <= t < min(t0 + nt, clip_frames[b]), r in clip b }.  One workgroup
 *                               owns each counter, no atomics.
 *   sfsn_zero_tail_frames       x [B][rows][T][width] float: frames t >= clip_frames[b] := 0 (each element stored once; the rest
 *                               of x is not touched).  T * width < 2^31.
 *   sfsn_fullband_proj_deepfilter_ragged  sfsn_fullband_proj_deepfilter (csrc/sfsn_fullband.hip) with T_b = clip_frames[b] clamped into
 *                               [0, T].  Frames t0 <= t < min(t0 + nt, T_b): enh_ri, enh_mag and proj of clip b have the bits of the
 *                               sibling on that clip alone (every clip_frames[b] = T: of the sibling on the batch).  Frames
 *                               max(t0, T_b) <= t < t0 + nt: enh_ri and enh_mag (where given) are stored as 0, once, and proj is not
 *                               written; nothing of stft_ri or spikes_i8 at frames >= T_b is read (skipped, not multiplied by zero:
 *                               the padding may hold NaN), and a 16-frame tile wholly past T_b loads no weights and issues no MFMA.
 *                               Outside [t0, t0 + nt) nothing is touched.  The sibling's SFSN_EINVAL / SFSN_EUNSUPPORTED cases.
 *                               (Added without an ABI bump: no struct or signature changed.)
 * ---------------------------------------------------------------------------------------------------- */
int sfsn_stft_ragged(const float* wave /* [B][L] */, int B, int L, int n_fft, int hop, const float* window,
                     float* stft_ri /* [B][n_fft/2+1][T][2] */, int T, const int32_t* clip_len /* device [B] */, void* stream);
int sfsn_istft_ragged(const float* stft_ri /* [B][n_fft/2+1][T][2] */, int B, int T, int n_fft, int hop, const float* window,
                      float* wave /* [B][length] */, int length, const int32_t* clip_frames /* device [B] */,
                      const int32_t* clip_len /* device [B] */, void* stream);
int sfsn_laplace_means_ragged(const float* stft_ri, const float* fb_tbf, int B, int F, int T, int FB, float fdrc,
                              const sfsn_feature_group* groups /* host, only geometry fields are read */, int n_groups,
                              const int32_t* clip_frames /* device [B] */, float* mu_out, float* scratch, void* stream);
int sfsn_gaussian_stats_ragged(const float* stft_ri, const float* fb_tbf, int B, int F, int T, int FB, float fdrc,
                               const sfsn_feature_group* groups /* host, only geometry fields are read */, int n_groups,
                               const int32_t* clip_frames /* device [B] */, float* mu_out, float* sd_out, float* scratch, void* stream);
int sfsn_spike_count_rows_ragged(const sfsn_row_count* tensors /* host */, int n_tensors, int t0, int nt,
                                 const int32_t* clip_frames /* device [B] */, int B, void* stream);
int sfsn_zero_tail_frames(float* x /* [B][rows][T][width] */, int B, int rows, int T, int width,
                          const int32_t* clip_frames /* device [B] */, void* stream);
int sfsn_fullband_proj_deepfilter_ragged(const float* stft_ri /* [B][F][T][2] */, const int8_t* spikes_i8 /* [T][B][pad64(H)] */, int H,
                                         const int8_t* w_packed, const float* w_dq, const float* bias, int act, int B, int F, int T,
                                         int S, int df, float* proj /* [T][B][2 df S F], nullable */,
                                         float* enh_ri /* [B][S][F][T][2] */, float* enh_mag /* [B][S][F][T], nullable */, int t0,
                                         int nt, const int32_t* clip_frames /* device [B] */, void* stream);

/* ----------------------------------------------------------------------------------------------------
 * Scoring a ragged batch: sfsn_pit_sdr with per-clip lengths, plus the clips' own losses and audiozen.metric.SISDR of the matched
 * rows (csrc/sfsn_pit.hip).  est, ref [clips][sources][n_samples], n_samples the padded row length; clip b is its samples
 * [0, L_b), L_b = clip_len[b] clamped into [0, n_samples] on the device.  The ragged contract above holds: pair[b], perm[b],
 * clip_loss[b], the pairwise-mode rows of grad_est and reordered[b][:, :L_b] have the BITS of sfsn_pit_sdr on a contiguous copy of
 * that clip alone (clips = 1, n_samples = L_b), and with every clip_len[b] = n_samples every output has the bits of sfsn_pit_sdr on
 * the batch.
 *   own length   nothing at or past L_b is read, from est or from ref (the padding may hold anything, NaN included); the zero-mean
 *                divisor and every L of the formulas is L_b; the clip's sums run over its own ceil(L_b / 2048) chunk partials in
 *                chunk order; a workgroup whose chunk starts at or past L_b adds no partial and, in the second launch, writes zeros
 *   tails        grad_est and reordered are +0.0f from sample L_b to n_samples; every element of both is stored exactly once
 *   clip_loss    [clips], PIT mode, nullable: min_p loss_p[b] in fp32
 *   loss         [1]: the mean of the clips' minima, every clip weighted EQUALLY (added in clip order in fp64): what averaging the
 *                one-clip calls gives, not a length-weighted mean.  The PIT-mode gradient's weight is 1 / (clips S).
 *   si_sdr       [clips][sources], PIT mode, nullable: audiozen.metric.SISDR (metric.py:67-101) of ref[b][j] against its matched
 *                estimate est[b][perm[b][j]]: both minus their own mean over L_b whatever zero_mean says, eps' = 2^-23
 *                (torch.finfo(float32).eps), proj = (dot s + eps') / (|s|^2 + eps') per sample,
 *                10 log10((sum proj^2 + eps') / (sum noise^2 + eps') + eps').  Evaluated in fp64 from the centred sums of the first
 *                launch (sum proj^2 = (dot^2 n + L_b eps'^2) / (n + eps')^2, sum a proj = dot^2 / (n + eps'),
 *                sum noise^2 = sum a^2 - 2 sum a proj + sum proj^2) by the workgroup that writes pair; rounded to fp32 once.
 *   L_b < 2      gives whatever the formulas give for that clip (L_b = 0: NaN) and never an out-of-range access.
 * Scratch is sfsn_pit_sdr_scratch_bytes(clips, sources, n_samples).  Modes, alignment (clip_len, clip_loss and si_sdr included),
 * sources <= 4 and the 32-bit limit are sfsn_pit_sdr's.  Checked before any launch, in addition to sfsn_pit_sdr's conditions: a NULL
 * clip_len; clip_loss or si_sdr given together with pair_cot -> SFSN_EINVAL.  Two plain launches, deterministic, capturable.
 * ---------------------------------------------------------------------------------------------------- */
int sfsn_pit_sdr_ragged(const float* est, const float* ref /* [clips][sources][n_samples] */, int clips, int sources, int n_samples,
                        const int32_t* clip_len /* device [clips] */, int zero_mean, float eps, const float* pair_cot /* nullable */,
                        float* pair /* [clips][S][S] */, int32_t* perm /* [clips][S] */, float* clip_loss /* nullable [clips] */,
                        float* loss /* [1] */, float* grad_est /* nullable */, float* reordered /* nullable */,
                        float* si_sdr /* nullable [clips][S] */, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SFSN_H */
