/*
 * rvcmi.h -- C ABI of the MI355X-native RVC hot path (librvcmi.so).
 *
 * The reference (fumiama/Retrieval-based-Voice-Conversion-WebUI) has no C ABI of its own: its
 * boundary for this path is two Python objects,
 *
 *   (1) the faiss index held by the pipeline
 *         faiss.read_index(path)                infer/modules/vc/pipeline.py:214, infer/lib/rtrvc.py:56
 *         index.reconstruct_n(0, index.ntotal)  infer/modules/vc/pipeline.py:215, infer/lib/rtrvc.py:57
 *         index.search(npy, k=8)                infer/modules/vc/pipeline.py:126, infer/lib/rtrvc.py:172
 *         the (1/score)^2 blend                 infer/modules/vc/pipeline.py:129-138
 *   (2) the generator module `net_g.dec`
 *         NSFGenerator.forward(x, f0, g, n_res) rvc/layers/nsf.py:145-191
 *         Generator.forward(x, g, n_res)        rvc/layers/generators.py:70-98
 *         built / weight-norm-folded by         rvc/synthesizer.py:10-28
 *
 * Each entry point below names the reference call it stands in for.  The Python mirror of those
 * objects (package `retrieval-based-voice-conversion-webui_amd`, imported as `rvc_amd`) binds this
 * header with ctypes; INTEGRATION.md shows the two-line patch on the reference side.
 *
 * Conventions
 *   - extern "C", opaque handles, plain pointers and sizes, no C++/torch types.
 *   - every function returns 0 on success and a negative rvcmi_status on failure; the message is
 *     available from rvcmi_last_error() (thread-local).  Nothing throws across the ABI.
 *   - all `*_dev` pointers are DEVICE pointers owned by the caller (hipMalloc / torch.cuda);
 *     all work is enqueued on the caller's `stream` (a hipStream_t passed as void*); no hidden
 *     synchronisation, no allocation after create  =>  every forward/search is hipGraph-capturable.
 *   - handles are immutable after create except for their private workspace: one in-flight
 *     forward per handle (use one handle per stream for concurrency).
 */
#ifndef RVCMI_H
#define RVCMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version.  2: rvcmi_nsf_forward takes lengths_dev as its 4th argument (ragged batches).  A binding must compare
 * rvcmi_version() with the RVCMI_VERSION it was written against before its first call: a v1 caller on a v2 library would
 * shift every pointer by one.                                                                                              */
#define RVCMI_VERSION 2

typedef enum {
    RVCMI_OK = 0,
    RVCMI_ERR_INVALID = -1,     /* bad argument / unsupported configuration            */
    RVCMI_ERR_HIP = -2,         /* a HIP runtime call failed                            */
    RVCMI_ERR_IO = -3,          /* file missing / truncated / not an IVF-Flat L2 index  */
    RVCMI_ERR_NOMEM = -4,       /* shape exceeds the handle's max_B / max_T             */
    RVCMI_ERR_MISSING = -5      /* a required weight tensor was not supplied            */
} rvcmi_status;

const char* rvcmi_last_error(void);
int rvcmi_version(void);

/* ------------------------------------------------------------------------------------------- */
/* Generator (NSF-HiFi-GAN)                                                                      */
/* ------------------------------------------------------------------------------------------- */

#define RVCMI_MAX_UPS 8
#define RVCMI_MAX_RB 4
#define RVCMI_MAX_DIL 4

typedef enum {
    RVCMI_OPERAND_F32 = 0,   /* exact-fp32 VALU convolutions (bring-up / highest fidelity) */
    RVCMI_OPERAND_BF16 = 1,  /* bf16 MFMA operands, fp32 accumulate + fp32 residual stream */
    RVCMI_OPERAND_F16 = 2,   /* fp16 MFMA operands, fp32 accumulate + fp32 residual stream */
    RVCMI_OPERAND_F16X2 = 3  /* FRONT ONLY (rvcmi_front_config; rvcmi_nsf_create rejects it): every MFMA operand a (hi, lo) pair of fp16
                              * values, three fp16 MFMAs per k-step, fp32 accumulate -- fp32-grade enc_p / flow on the fp16 matrix cores.
                              * One launch form per layer: rvcmi_front_set_option returns RVCMI_ERR_INVALID for a key / value that
                              * selects a fused or split form (FR_NO_FFN_FUSION 0, FR_FFN_SPLIT != 0, FR_WN_SPLIT != 1, FR_STAMPS != 0). */
} rvcmi_operand;

/* Mirrors the positional `cpt["config"]` list consumed by rvc/synthesizer.py:10-22
 * (written by infer/lib/train/process_ckpt.py:23-42). */
typedef struct {
    int inter_channels;                       /* 192                                          */
    int upsample_initial_channel;             /* 512                                          */
    int gin_channels;                         /* 256 (0 = no speaker conditioning)            */
    int sr;                                   /* 32000 / 40000 / 48000                        */
    int use_f0;                               /* 1 = NSFGenerator, 0 = Generator              */
    int n_ups;
    int upsample_rates[RVCMI_MAX_UPS];
    int upsample_kernel_sizes[RVCMI_MAX_UPS];
    int n_resblock_kernels;                   /* 3                                            */
    int resblock_kernel_sizes[RVCMI_MAX_RB];
    int n_dilations[RVCMI_MAX_RB];
    int resblock_dilation_sizes[RVCMI_MAX_RB][RVCMI_MAX_DIL];
    int operand;                              /* rvcmi_operand                                */
} rvcmi_nsf_config;

/* One fp32 host tensor; `name` is the state_dict key under "dec." after remove_weight_norm()
 * (e.g. "ups.0.weight", "resblocks.3.convs1.0.bias").                                         */
typedef struct {
    const char* name;
    const float* data;      /* host pointer, C-contiguous                                       */
    int ndim;
    int64_t shape[4];
} rvcmi_tensor;

typedef struct rvcmi_nsf rvcmi_nsf;

/* Stands in for rvc/synthesizer.py:10-28 (construction + weight prep of `net_g.dec`).
 * Packs the weights into MFMA fragment order on `device` and allocates a workspace sized for
 * max_B utterances of max_T frames.                                                            */
int rvcmi_nsf_create(const rvcmi_nsf_config* cfg, const rvcmi_tensor* weights, int n_weights,
                     int device, int max_B, int max_T, rvcmi_nsf** out);
int rvcmi_nsf_destroy(rvcmi_nsf* h);

/* Stands in for NSFGenerator.forward (rvc/layers/nsf.py:145-191) / Generator.forward
 * (rvc/layers/generators.py:70-98).
 *   x_dev      [B, inter, T] fp32 (the reference's channel-first layout)
 *   f0_dev     [B, T] fp32 Hz, 0 = unvoiced; NULL iff use_f0 == 0
 *   g_dev      [B, gin] fp32 speaker embedding (emb_g(sid)), or NULL
 *   noise_dev  [B, T*upp] fp32 N(0,1) -- the draw the reference makes at generators.py:192 --
 *              or NULL for zeros.  (The reference's rand_ini at :164-166 is forced to 0 for the
 *              only harmonic there is, so it never reaches the output.)
 *   n_res      -1 = none; otherwise the realtime "return_length2" resample target, nsf.py:155-162
 *   out_dev    [B, T_out*upp] fp32, T_out = n_res if n_res >= 0 else T
 *   lengths_dev  NULL, or int32 [B] on the device with 1 <= lengths[b] <= T: a RAGGED batch.  Item b is
 *              computed exactly as a separate call with T = lengths[b] on its first lengths[b] frames (lengths[b] * upp
 *              noise samples) would compute it: every layer zero-pads its input behind the item's own last row, so the
 *              segments of a long file (infer/modules/vc/pipeline.py:205-209, 301-343) and the utterances of a folder
 *              (infer/modules/vc/modules.py:201-266 vc_multi) convert in ONE call with the waveform of sequential calls.
 *              Output samples [lengths[b] * upp, T * upp) of item b are zero.  Not combinable with n_res.
 */
int rvcmi_nsf_forward(rvcmi_nsf* h, int B, int T, const int* lengths_dev, const float* x_dev, const float* f0_dev,
                      const float* g_dev, const float* noise_dev, int n_res, float* out_dev,
                      void* stream);

/* rvcmi_nsf_forward with a realtime resample target PER ITEM (the bank's formant shift per session: return_length2 of rtrvc.py:191
 * differs between the sessions of one batch).
 *   n_res_dev  int32 [B] on the device, 1 <= n_res[b] <= n_res_max; the caller vouches for the values (they are not read back)
 *   out_dev    [B, n_res_max * upp] fp32
 * Item b is computed exactly as rvcmi_nsf_forward(h, 1, T, NULL, x[b], f0[b], g[b], noise[b], n_res[b], ...) computes it: the
 * excitation over all T input frames, then it and x interpolated to n_res[b] frames (an item with n_res[b] == T is not
 * interpolated, as there), the layers behind as a ragged item of n_res[b] frames.  Output samples [n_res[b] * upp, n_res_max * upp)
 * of item b are zero.  n_res_max > max_T: RVCMI_ERR_NOMEM; B < 1, n_res_max < 1, a null n_res_dev: RVCMI_ERR_INVALID.  No
 * allocation, no synchronisation, no host read of n_res_dev.  Serves no debug tap. */
int rvcmi_nsf_forward_nres(rvcmi_nsf* h, int B, int T, int n_res_max, const int* n_res_dev, const float* x_dev, const float* f0_dev,
                           const float* g_dev, const float* noise_dev, float* out_dev, void* stream);

int rvcmi_nsf_upp(const rvcmi_nsf* h);               /* prod(upsample_rates)                    */
size_t rvcmi_nsf_workspace_bytes(const rvcmi_nsf* h);

/* Stage taps for bring-up and per-layer parity tests (not on the product path): runs the forward
 * up to the named activation and copies it to the host in the reference's channel-first layout
 * [B, C, L].  `what`: "har" ([B,1,T*upp]), "pre", "up<i>" (after ups+noise_convs), "stage<i>"
 * (the SUM of the stage's ResBlocks, i.e. before the /num_kernels of nsf.py:186).
 * Synchronises the stream.                                                                       */
int rvcmi_nsf_debug_forward(rvcmi_nsf* h, int B, int T, const float* x_dev, const float* f0_dev,
                            const float* g_dev, const float* noise_dev, int n_res, const char* what,
                            float* out_host, size_t capacity_floats, int64_t shape_out[3],
                            void* stream);

/* Per-kernel HIP-event timing (bench.py's roofline leg).  When enabled, every launch of the
 * forward is bracketed by hipEvents on the caller's stream; not usable under graph capture.
 * rvcmi_nsf_profile_read returns, for kernel class i < *n, its name, launch count, total ms
 * and algorithmic flops/bytes accumulated since the last reset.                                */
typedef struct {
    char name[48];
    int64_t launches;
    double ms;
    double flops;      /* 2*Cin*Cout*k*L summed over launches                                  */
    double bytes;      /* algorithmic bytes moved to/from global memory                        */
} rvcmi_kernel_stat;
int rvcmi_nsf_profile_enable(rvcmi_nsf* h, int enable);
/* Development / test options of ONE handle (kernel-family forcing, tile heights, phase stamps, timing ablations).  A handle
 * reads the environment variables RVCMI_<KEY> exactly once, when it is created; afterwards only this call changes an option
 * (value NaN = back to the default).  The forward / search paths never read the environment.  Keys: see the option comments
 * of the handle structs in csrc/nsf.hip, csrc/rb_stream.hpp, csrc/front.hip, csrc/ivf.hip.  Not part of the reference's
 * surface; product code does not call these. */
int rvcmi_nsf_set_option(rvcmi_nsf* h, const char* key, double value);
int rvcmi_nsf_profile_read(rvcmi_nsf* h, rvcmi_kernel_stat* stats, int capacity, int* n, int reset);

/* How the last forward of a handle ran each upsampling stage's ResBlocks (tests and tools; product code does not call this).
 * One record per stage the forward reached, written by the forward itself from the values it launched with.  Every field is an int. */
enum { RVCMI_RB_F32_CHAIN = 0, RVCMI_RB_SPLIT = 1, RVCMI_RB_STREAM = 2, RVCMI_RB_FULL = 3, RVCMI_RB_PAIR = 4 };
typedef struct {
    int path;          /* RVCMI_RB_*: conv by conv in fp32 / output-channel-split convs per pair level / whole ResBlocks on the streaming
                        * kernel / whole ResBlocks fused, one launch / one launch per pair level                                       */
    int C;             /* channels of the stage                                                                                        */
    int B, rows;       /* batch items, rows per item (T x the upsample rates so far)                                                   */
    int x0_half;       /* the upsampler's output, the ResBlocks' input, is stored as fp16                                              */
    int y_half;        /* the ResBlocks' output streams are stored as fp16                                                             */
    int tile_rows;     /* FULL, PAIR: rows a block computes (a ResBlock keeps tile_rows minus its halo of them)                        */
    int tile_waves;    /* FULL: waves per block                                                                                        */
    int n_rb;          /* STREAM, FULL, PAIR: ResBlocks described below, in launch order (largest kernel size first)                   */
    int k[RVCMI_MAX_RB];          /* kernel size                                                                                       */
    int tiles[RVCMI_MAX_RB];      /* FULL, PAIR: tiles per item (PAIR: of every pair level); STREAM: strips per item                   */
    int strip_len[RVCMI_MAX_RB];  /* STREAM: rows per strip, strips x strip_len >= rows                                                */
    int stream_nj;     /* STREAM: the kernel advances 32 x stream_nj rows per step                                                     */
    int stream_mfma;   /* STREAM: MFMA shape of its K loops, 16 (v_mfma_f32_16x16x32) or 32 (32x32x16)                                 */
    int stream_fill_skip;  /* STREAM: a strip's first step skips its pipeline-fill column tiles                                        */
    int pair_streamed; /* PAIR: bit m set = pair level m ran on the streaming kernel's pair-level form                                 */
    int num_cus;       /* compute units the planner saw                                                                                */
} rvcmi_nsf_stage_plan;
/* Copies the *n records of the last forward to out[0 .. *n).  A capacity smaller than the number of records is
 * RVCMI_ERR_INVALID and writes nothing, neither out nor *n (RVCMI_MAX_UPS always suffices).  A handle that has not run a forward reports *n = 0.
 *   - A forward that ended at a debug tap (rvcmi_nsf_debug_forward) reports the stages planned up to the tap; of a stage whose
 *     ResBlocks did not run ("up<i>") the fields from tile_rows to pair_streamed are zero.
 *   - Replaying a captured graph runs no host code of the forward: the record stays that of the capturing call.               */
int rvcmi_nsf_last_plan(const rvcmi_nsf* h, rvcmi_nsf_stage_plan* out, int capacity, int* n);

/* ------------------------------------------------------------------------------------------- */
/* Synthesizer front: enc_p + prior sampling + flow^-1              */
/* ------------------------------------------------------------------------------------------- */

/* What SynthesizerTrnMsNSFsid.infer (rvc/layers/synthesizers.py:160-203) runs before self.dec:
 *     m_p, logs_p, x_mask = self.enc_p(phone, pitch, phone_lengths, flow_head)   encoders.py:134-159
 *     z_p = (m_p + exp(logs_p) * randn_like(m_p) * 0.66666) * x_mask             synthesizers.py:182-183
 *     z   = self.flow(z_p, x_mask, g=g, reverse=True)                            residuals.py:319-321
 * With this handle and rvcmi_nsf the whole `infer` runs without a torch op in between.
 * Hyper-parameters are the positional config list of a checkpoint (configs/v2/48k.json:19-27). */
typedef struct {
    int in_channels;          /* 768 (v2, SynthesizerTrnMs768NSFsid) or 256 (v1)                */
    int inter_channels;       /* 192                                                            */
    int hidden_channels;      /* 192                                                            */
    int filter_channels;      /* 768                                                            */
    int n_heads;              /* 2                                                              */
    int n_layers;             /* 6                                                              */
    int kernel_size;          /* FFN kernel, 3                                                  */
    int window_size;          /* relative-attention window, 10 (encoders.py:21)                 */
    int gin_channels;         /* 256                                                            */
    int use_f0;               /* emb_pitch present (encoders.py:107-108)                        */
    int flow_n_flows;         /* 4  (residuals.py:275)                                          */
    int flow_n_layers;        /* 3  (synthesizers.py:111-113)                                   */
    int flow_kernel_size;     /* 5                                                              */
    int flow_dilation_rate;   /* 1                                                              */
    int operand;              /* RVCMI_OPERAND_F16 / _BF16 / _F16X2 (MFMA operands; everything else fp32) */
} rvcmi_front_config;

typedef struct rvcmi_front rvcmi_front;

/* Stands in for the enc_p / flow part of get_synthesizer (rvc/synthesizer.py:10-28).  `weights` are fp32 HOST
 * tensors named by the keys of net_g.state_dict() AFTER remove_weight_norm(): "enc_p.emb_phone.weight",
 * "enc_p.encoder.attn_layers.0.conv_q.weight", "enc_p.encoder.attn_layers.0.emb_rel_k", ...,
 * "enc_p.proj.weight", "flow.flows.0.pre.weight", "flow.flows.0.enc.in_layers.0.weight", ...,
 * "flow.flows.6.post.bias".  The channel Flip modules are folded into the packed weights.       */
int rvcmi_front_create(const rvcmi_front_config* cfg, const rvcmi_tensor* weights, int n_weights, int device,
                       int max_B, int max_T, rvcmi_front** out);
int rvcmi_front_destroy(rvcmi_front* h);

/* One pass.  phone_dev [B][T][in_channels] fp32 (features after the x2 interpolation, pipeline.py:146-150);
 * pitch_dev [B][T] int64 coarse bins or NULL (no-f0 models); lengths_dev [B] int64 (phone_lengths) or NULL = all T;
 * g_dev [B][gin] fp32 = emb_g(sid); noise_dev [B][inter][T - flow_head] fp32 standing for randn_like(m_p);
 * flow_head = max(skip_head - 24, 0) for the realtime partial decode (synthesizers.py:175-181), else 0.
 * z_out_dev [B][inter][T - flow_head] fp32 = z * x_mask, the layout rvcmi_nsf_forward takes as x_dev.  */
int rvcmi_front_forward(rvcmi_front* h, int B, int T, const float* phone_dev, const int64_t* pitch_dev,
                        const int64_t* lengths_dev, const float* g_dev, const float* noise_dev, int flow_head,
                        float* z_out_dev, void* stream);
size_t rvcmi_front_workspace_bytes(const rvcmi_front* h);

/* Test hook: stop after an internal stage and copy it to the host, channels-last [B][T'][192].
 * what: "emb", "attn0".."attn5" (after an encoder layer's attention half: LayerNorm 1), "layer0".."layer5" (encoder stream), "z_p", "flow3".."flow0" (flow stream after a coupling). */
int rvcmi_front_debug_forward(rvcmi_front* h, int B, int T, const float* phone_dev, const int64_t* pitch_dev,
                              const int64_t* lengths_dev, const float* g_dev, const float* noise_dev, int flow_head,
                              const char* what, float* out_host, size_t capacity_floats, int64_t shape_out[3],
                              void* stream);
int rvcmi_front_set_option(rvcmi_front* h, const char* key, double value);
int rvcmi_front_profile_enable(rvcmi_front* h, int enable);
int rvcmi_front_profile_read(rvcmi_front* h, rvcmi_kernel_stat* stats, int capacity, int* n, int reset);

/* ------------------------------------------------------------------------------------------- */
/* IVF-Flat retrieval (faiss IndexIVFFlat, METRIC_L2)                                           */
/* ------------------------------------------------------------------------------------------- */

typedef struct rvcmi_ivf rvcmi_ivf;

/* faiss.read_index(path)  (pipeline.py:214).  Parses the IwFl/IxF2/ilar on-disk layout.       */
int rvcmi_ivf_create_from_file(const char* path, int device, rvcmi_ivf** out);
/* index.train(big_npy) + index.add(big_npy)  (web.py:554-563), on the GPU:
 *   k-means for the nlist centroids (niter Lloyd iterations from nlist seeded training vectors; every assignment
 *   is the exact fp64 nearest centroid, computed by the search path's own coarse kernels; empty lists are re-seeded
 *   by splitting the largest one), then every vector goes to the list of its nearest centroid, ids = row numbers
 *   in add order (rvcmi_ivf_train's centroids followed by the device-side placement of rvcmi_ivf_add).  x_host [n,d] fp32 HOST (what np.load gives).  nprobe = 1 (web.py:552).  objective_out
 *   (optional, niter+1 doubles) receives the sum of squared distances at every assignment step.
 *   faiss' own k-means (its RNG, sub-sampling and split heuristics) is not reproduced: retrieval semantics do not
 *   depend on how the centroids were found, and the reference pins nothing here.                      */
int rvcmi_ivf_build(int d, int64_t n, const float* x_host, int64_t nlist, int niter, uint64_t seed, int device,
                    double* objective_out, rvcmi_ivf** out);
/* The large-set branch of the index recipe (web.py:522-536: more than 2e5 feature rows are replaced by 10k k-means centres,
 * sklearn MiniBatchKMeans there) without building an index: the SAME Lloyd iterations as rvcmi_ivf_build -- niter updates
 * from k seeded training vectors, exact fp64 assignments, a cluster that loses all its points is re-seeded by splitting the
 * largest one, so all k centres are valid -- and only the centres come back.  x_host [n,d] fp32 HOST, centroids_out_host
 * [k,d] fp32 HOST, objective_out optional (niter doubles).                                                              */
int rvcmi_kmeans(int d, int64_t n, const float* x_host, int64_t k, int niter, uint64_t seed, int device, double* objective_out,
                 float* centroids_out_host);
/* index.train(big_npy) alone  (web.py:553-554; tools/cmd/train-index-v2.py:56-57): the k-means of rvcmi_kmeans, returned as a
 * trained, EMPTY index (ntotal 0, nprobe 1) -- what the reference writes as trained_IVF*.index (web.py:556-559) before it adds.
 * x_host [n,d] fp32 HOST, n >= nlist; objective_out optional (niter doubles, as rvcmi_kmeans).                              */
int rvcmi_ivf_train(int d, int64_t n, const float* x_host, int64_t nlist, int niter, uint64_t seed, int device,
                    double* objective_out, rvcmi_ivf** out);
/* index.add(x)  (web.py:561-563: `for i in range(0, N, 8192): index.add(big_npy[i : i + 8192])`): appends n rows [n,d] fp32 with
 * ids ntotal .. ntotal + n - 1 (faiss' sequential add; add_with_ids is not offered).  x is a DEVICE pointer on the index's device
 * when x_on_device != 0, else a host pointer (copied up once).  Every row goes to the list of its exact nearest centroid -- the
 * assignment of rvcmi_ivf_search's coarse step and of rvcmi_ivf_build, ties to the lowest list -- behind the list's old rows, new
 * rows in ascending id order: the result is a function of (old index, x) alone, and adding in batches equals adding at once.
 * Assignment, counting, the new list offsets, the move of the old rows and the placement of the new ones all run on the device.
 * The index moves to a NEW blob of the size for ntotal + n rows: the pointer rvcmi_ivf_blob reports CHANGES; the old blob is freed
 * if the handle owned it, a blob adopted by rvcmi_ivf_create_from_blob without ownership is left untouched (the handle owns the
 * new one).  Peak device memory: old blob + new blob + x (+ the assignment scratch).  The search workspace reserved so far is
 * rebuilt for the new rows before the call returns.  A build-time call: it allocates and synchronises `stream` -- never call it
 * under stream capture, nor concurrently with a search on the same handle.
 * n == 0 is a no-op; an untrained / foreign handle, a null x with n > 0, a negative n or one that overflows: RVCMI_ERR_INVALID. */
int rvcmi_ivf_add(rvcmi_ivf* h, int64_t n, const float* x, int x_on_device, void* stream);
/* faiss.write_index(index, path)  (web.py:571) -- so indices round-trip with stock RVC.       */
int rvcmi_ivf_write_file(const rvcmi_ivf* h, const char* path);

/* Direct construction from host arrays (what index.train()+index.add() leave behind, web.py:553-563):
 * centroids [nlist,d], list_offsets [nlist+1], ids [n] and vecs [n,d] in list-major order.     */
int rvcmi_ivf_create(int d, int64_t n, int64_t nlist, int nprobe, const float* centroids,
                     const int64_t* list_offsets, const int64_t* ids, const float* vecs,
                     int device, rvcmi_ivf** out);
int rvcmi_ivf_destroy(rvcmi_ivf* h);

int rvcmi_ivf_d(const rvcmi_ivf* h);
int64_t rvcmi_ivf_ntotal(const rvcmi_ivf* h);            /* index.ntotal                         */
int64_t rvcmi_ivf_nlist(const rvcmi_ivf* h);
int rvcmi_ivf_nprobe(const rvcmi_ivf* h);                /* extract_index_ivf(index).nprobe      */
int rvcmi_ivf_set_nprobe(rvcmi_ivf* h, int nprobe);      /* web.py:551-552                       */

/* Pre-size the search workspace for up to max_nq queries (searches with nq above the current
 * reservation grow it, which allocates: reserve before hipGraph capture).                      */
int rvcmi_ivf_reserve(rvcmi_ivf* h, int64_t max_nq);

/* index.search(x, k)  (pipeline.py:126): q_dev [nq,d] fp32 -> D_dev [nq,k] fp32 squared-L2
 * ascending, I_dev [nq,k] int64 (-1 / FLT_MAX padded).  k <= 8.  Distances are evaluated in fp64
 * on the fp32 inputs; ties break to the lowest id.                                             */
int rvcmi_ivf_search(rvcmi_ivf* h, int64_t nq, const float* q_dev, int k, float* D_dev,
                     int64_t* I_dev, void* stream);

/* search + pipeline.py:129-138 fused, everything device-resident:
 *   w = (1/D)^2 / sum; feats = (sum_k w_k * big_npy[I_k]) * index_rate + (1-index_rate) * feats
 * feats_dev [nq,d] fp32 is updated in place.  skip_if_short != 0 reproduces the realtime guard
 * `if (ix >= 0).all()` of infer/lib/rtrvc.py:173 (per call, not per row).                       */
int rvcmi_ivf_search_blend(rvcmi_ivf* h, int64_t nq, float* feats_dev, float index_rate, int k,
                           int skip_if_short, void* stream);

/* rvcmi_ivf_search_blend followed by what Pipeline.vc does next (pipeline.py:140-159), in one pass over the rows:
 *   F.interpolate(scale_factor=2) (nearest: out frame t <- row t/2), truncation to p_len <= 2*nq, and -- when
 *   pitchf_dev is not NULL (the `protect < 0.5` branch) -- feats*pitchff + feats0*(1-pitchff) with
 *   pitchff = pitchf[t] < 1 ? protect : 1.  feats_dev [nq,d] is NOT modified; out_dev is [p_len,d].            */
int rvcmi_ivf_search_blend_expand(rvcmi_ivf* h, int64_t nq, const float* feats_dev, float index_rate, int k,
                                  int skip_if_short, const float* pitchf_dev, float protect, int64_t p_len,
                                  float* out_dev, void* stream);

/* rvcmi_ivf_search_blend_expand for a bank of S realtime sessions that share the index (feats_dev [S, nq, d], pitchf_dev
 * [S, p_len] or NULL, out_dev [S, p_len, d], all contiguous): per session, rows [0, skip_rows) are expanded un-blended and rows
 * [skip_rows, nq) are searched and blended -- what two single-session calls on the two row ranges compute, bit for bit.  All
 * S * (nq - skip_rows) searched rows go through ONE search; the launch count does not depend on S.  The realtime guard
 * (skip_if_short != 0; rtrvc.py:172-180 is a per-call condition, and a call is one talker's block) is evaluated PER SESSION:
 * the result ids are reduced into one flag per session after the search, so a session whose rows probe a list shorter than k
 * keeps its own features and leaves the others' blend alone.  1 <= S <= 65535, 0 <= skip_rows <= nq, p_len <= 2 * nq.
 * The handle keeps the packed query rows and the flags (grown on demand, like rvcmi_ivf_reserve).                            */
int rvcmi_ivf_search_blend_expand_batch(rvcmi_ivf* h, int S, int64_t nq, int64_t skip_rows, const float* feats_dev,
                                        float index_rate, int k, int skip_if_short, const float* pitchf_dev, float protect,
                                        int64_t p_len, float* out_dev, void* stream);

/* rvcmi_ivf_search_blend_expand_batch with the four retrieval controls PER SESSION (the GUI's index_rate slider and RVC.infer's protect,
 * gui.py:676-679, rtrvc.py:167-185, 221-233).  Session s is described by sess[s]:
 *   index_rate   its blend weight;   slot   >= 0: the session is searched and blended, and this is its position among the sessions
 *   that are (they count up from 0 in session order); -1: it is not -- its rows are expanded un-blended, the BITS of its input rows
 *   (never acc * 0 + 1 * f: a -0.0 stays -0.0, and nothing of the index reaches it);   protect / protect_on   the protect mix of the
 *   session, applied iff protect_on (then pitchf_dev must not be NULL); protect_on == 0 gives o = x, as a NULL pitchf_dev does.
 * Only the sessions with a slot contribute rows to the ONE search: their rows [skip_rows, nq) are packed by slot, the realtime guard
 * (skip_if_short) is reduced per packed slot, and the blend maps session -> slot.  With no such session nothing is searched.  Row s of
 * out_dev equals rvcmi_ivf_search_blend_expand_batch at S = 1 on session s's rows with its values (or rvcmi_glue_expand_protect_batch
 * for a session without a slot) bit for bit: the same device bodies.  The launch count depends on neither S nor on which sessions
 * blend.  h may be NULL -- a bank without an index that has a protect per session: then every slot must be -1, and d is the feature
 * width; with a handle d must be the index's.  The values are given twice, as rvcmi_glue_rmvpe_f0_ragged takes its rows: sess_host is
 * checked (and the search planned from it) before anything is launched, sess_dev -- the same bytes in device memory -- is what the
 * kernels read.  Enqueue-only: no allocation beyond the handle's grow-on-demand buffers, no synchronisation, no device memory read by
 * the host.  RVCMI_ERR_INVALID, nothing launched: S outside [1, 65535], nq < 1, skip_rows outside [0, nq], p_len outside [0, 2 nq], a
 * value that is not finite, slots that do not count up, a slot without a handle, protect_on without pitchf_dev, d != the index's.
 * The `ivf_blend_x2` profile record carries flops = 2 * rows * k * d with rows = the rows actually searched.                          */
typedef struct {
    float index_rate;    /* the session's blend weight                                            */
    float protect;       /* the session's protect (used iff protect_on)                           */
    int32_t slot;        /* packed position among the blending sessions, or -1                    */
    int32_t protect_on;  /* 0 / 1: the protect mix applies                                        */
} rvcmi_session_blend;
int rvcmi_ivf_search_blend_expand_sessions(rvcmi_ivf* h, int S, int64_t nq, int d, int64_t skip_rows, const float* feats_dev,
                                           const rvcmi_session_blend* sess_host, const rvcmi_session_blend* sess_dev, int k,
                                           int skip_if_short, const float* pitchf_dev, int64_t p_len, float* out_dev, void* stream);

/* index.reconstruct_n(i0, n) -> out_host [n,d] rows in id order (pipeline.py:215).             */
int rvcmi_ivf_reconstruct_n(const rvcmi_ivf* h, int64_t i0, int64_t n, float* out_host);

/* The coarse centroids [nlist, d] (k-means cluster centres of a built index), e.g. as the 10k-centre reduction of a
 * large training set (web.py:522-536).                                                                             */
int rvcmi_ivf_centroids(const rvcmi_ivf* h, float* out_host);

/* Copies the packed index blob into caller-owned device memory (>= the size rvcmi_ivf_blob reports) on `stream`:
 * the source buffer of the RCCL broadcast of rvc_amd.dist.broadcast_index, made by this library's own HIP runtime.  */
int rvcmi_ivf_blob_copy(const rvcmi_ivf* h, void* dst_dev, size_t capacity, void* stream);

/* The whole index as ONE device blob (header + centroids + offsets + ids + vectors) so that a
 * single RCCL broadcast replicates it across the GPUs of a node.                */
int rvcmi_ivf_blob(const rvcmi_ivf* h, void** dev_ptr, size_t* bytes);
int rvcmi_ivf_create_from_blob(void* dev_ptr, size_t bytes, int device, int take_ownership,
                               rvcmi_ivf** out);

/* Per-phase HIP-event timing for bench.py (coarse / scan / blend), same contract as the nsf one. */
int rvcmi_ivf_set_option(rvcmi_ivf* h, const char* key, double value);
int rvcmi_ivf_profile_enable(rvcmi_ivf* h, int enable);
int rvcmi_ivf_profile_read(rvcmi_ivf* h, rvcmi_kernel_stat* stats, int capacity, int* n, int reset);

/* ------------------------------------------------------------------------------------------- */
/* Device-resident glue: stateless, everything on the caller's stream */
/* ------------------------------------------------------------------------------------------- */

/* The x2 interpolation + protect mix of pipeline.py:140-159 when NO index is used (index_rate == 0):
 * out[t] = feats[t/reps] (* pf + feats[t/reps] * (1 - pf) when pitchf_dev != NULL).
 * The bank form (rvcmi_glue_expand_protect_batch) at S = 1.                                        */
int rvcmi_glue_expand_protect(const float* feats_dev, int64_t nq, int d, int reps, const float* pitchf_dev,
                              float protect, int64_t p_len, float* out_dev, void* stream);

/* RMVPE salience [n,nbins=360] -> what Generator.calculate(..., "rmvpe") returns (rvc/f0/gen.py:43-123):
 *   _to_local_average_cents + _decode (rvc/f0/rmvpe.py:119-164), _resize_f0 to p_len and _interpolate_f0
 *   (rvc/f0/f0.py:31-78), post_process (rvc/f0/gen.py:10-41): key shift 2^(f0_up_key/12), mel binning to 1..255.
 * fp64 throughout, like numpy.  scratch_dev: n doubles.  pitch_dev [p_len] int64, pitchf_dev [p_len] fp32.
 * Any length: the single sequential pass keeps its work arrays in LDS up to n + p_len = 20480 frames and
 * in scratch_dev / pitch_dev beyond that (the reference computes f0 once per file, pipeline.py:260-266). */
int rvcmi_glue_rmvpe_f0(const float* salience_dev, int n, int nbins, float thred, int p_len, int f0_up_key,
                        double* scratch_dev, int64_t* pitch_dev, float* pitchf_dev, void* stream);
/* post_process only (f0 in Hz from any other estimator, fp64 [n]).                                 */
int rvcmi_glue_f0_post(const double* f0_dev, int n, int f0_up_key, int64_t* pitch_dev, float* pitchf_dev,
                       void* stream);
/* The same two with a fractional key (the realtime GUI's formant slider moves f0_up_key - formant_shift in steps of 0.05): the factor is
 * pow(2, f0_up_key / 12) in fp64, as the reference's post_process evaluates it for a python float.  The integer entry points above forward
 * here; for an integral key the factor is the same double.  A key that is not finite: RVCMI_ERR_INVALID.                              */
int rvcmi_glue_rmvpe_f0_key(const float* salience_dev, int n, int nbins, float thred, int p_len, double f0_up_key,
                            double* scratch_dev, int64_t* pitch_dev, float* pitchf_dev, void* stream);
int rvcmi_glue_f0_post_key(const double* f0_dev, int n, double f0_up_key, int64_t* pitch_dev, float* pitchf_dev,
                           void* stream);
/* The key factor of the entries above, pow(2, key / 12) in fp64 as the host evaluates it there (they call this function): what a caller
 * of rvcmi_glue_rmvpe_f0_ragged puts into rvcmi_f0_row.key_mul.  A key that is not finite: NaN, which that entry refuses.             */
double rvcmi_glue_f0_key_mul(double f0_up_key);

/* rvcmi_glue_rmvpe_f0_key for MANY sequences whose salience rows lie packed in one array [R, nbins] (rvcmi_gru_forward_ragged's layout;
 * rows between items are allowed and ignored), in TWO launches whatever nseq: the per-frame decode over all R rows, then one block per
 * item for resize + interpolation + post_process.  Item i is described by rows[i] and equals rvcmi_glue_rmvpe_f0_key on its rows
 * alone bit for bit, with key_mul = rvcmi_glue_f0_key_mul(its key).  The descriptors are given twice, as rvcmi_gru_forward_ragged takes
 * its offsets: rows_host is checked before anything is launched, rows_dev (the same bytes in device memory) is what the kernel reads.
 * scratch_dev: R doubles.  pitch_dev / pitchf_dev: out_len elements, item i at [out_off, out_off + p_len).
 * Work arrays: dynamic LDS sized for the largest item when (n + p_len) * 8 <= 160 KiB for EVERY item; otherwise every item works in
 * global memory, its rows of scratch_dev in place and its slice of pitch_dev -- the aliasing of the single call beyond 10240 frames.
 * Enqueue-only: no allocation, no synchronisation, no device memory read by the host.
 * RVCMI_ERR_INVALID, nothing launched: nseq < 1, an item with n < 1 or p_len < 1, a key_mul that is not finite and positive, source rows
 * outside [0, R), source ranges of two items that overlap (the global mode marks unvoiced frames in place), output ranges that overlap
 * or leave [0, out_len).                                                                                                              */
typedef struct {
    int64_t out_off;  /* first element of the item in pitch_dev / pitchf_dev */
    double key_mul;   /* rvcmi_glue_f0_key_mul(the item's key)               */
    int first_row;    /* first packed salience row of the item               */
    int n;            /* its frames (salience rows)                          */
    int p_len;        /* frames to return                                    */
    int reserved_;    /* 0                                                   */
} rvcmi_f0_row;
int rvcmi_glue_rmvpe_f0_ragged(const float* salience_dev, int64_t R, int nbins, int nseq, const rvcmi_f0_row* rows_host,
                               const rvcmi_f0_row* rows_dev, float thred, double* scratch_dev, int64_t* pitch_dev, float* pitchf_dev,
                               int64_t out_len, void* stream);

/* change_rms (infer/modules/vc/pipeline.py:26-46, called at :351 when rms_mix_rate != 1): mixes the loudness envelope of the
 * input (data1 at sr1 = 16000) into the converted audio data2 (sr2 = tgt_sr), IN PLACE on data2:
 *   data2 *= rms1^(1-rate) * max(rms2,1e-6)^(rate-1), rms_i = half-second frame RMS (librosa.feature.rms, centred, zero
 *   padded) linearly interpolated to len(data2).  scratch_dev: (1 + n1/(sr1/2)) + (1 + n2/(sr2/2)) floats.
 * The frame energies are summed in fp64; librosa sums in float32 in an order nothing in the reference pins.          */
int rvcmi_glue_change_rms(const float* data1_dev, int64_t n1, int sr1, float* data2_dev, int64_t n2, int sr2, float rate,
                          float* scratch_dev, void* stream);

/* pipeline.py:355-359: audio *= 32768 / max(1, abs(audio).max()/0.99), in place.  scratch_dev: 256 floats. */
int rvcmi_glue_scale_int16_range(float* audio_dev, int64_t n, float* scratch_dev, void* stream);

/* SOLA chunk stitching of the realtime path (gui.py:1057-1090): normalised cross-correlation
 * of infer_wav[: Lb + Ls] with sola_buffer [Lb] over offsets 0..Ls, argmax (first maximum), cut, cross-fade with the
 * sin^2 windows, out_block_dev [block_frame] <- result, sola_buffer_dev <- the next tail (in place).
 * offset_out_dev (optional) receives the chosen offset.  Needs Ls + block_frame + Lb <= n.
 * The bank form (rvcmi_glue_sola_batch) at S = 1 with contiguous rows: the same kernel, checks and limits. */
int rvcmi_glue_sola(const float* infer_wav_dev, int64_t n, float* sola_buffer_dev, int Lb, int Ls,
                    const float* fade_in_dev, const float* fade_out_dev, int block_frame, float* out_block_dev,
                    int* offset_out_dev, void* stream);

/* The GUI's phase-vocoder cross-fade (gui.py:27-49): out [n] <- phase_vocoder(a, b, fade_out, fade_in), all [n] fp32:
 *   w = sqrt(fade_out * fade_in);  Fa, Fb = rfft(a * w), rfft(b * w);  absab = |Fa| + |Fb| (doubled except DC / Nyquist);
 *   d = angle(Fb) - angle(Fa) wrapped by 2 pi floor(d / 2 pi + 0.5);
 *   out[t] = a fade_out^2 + b fade_in^2 + w / n * sum_k absab[k] cos((2 pi k + d[k]) t / n + angle(Fa)[k]).
 * Spectrum and synthesis in fp64 (an O(n * (n/2+1)) sum, not an inverse DFT).  A bin whose real and imaginary parts are both
 * exactly zero has phase 0.  n <= 4096, else RVCMI_ERR_INVALID.  scratch_dev: 3 * (n/2 + 1) doubles.
 * out_dev may not alias the inputs.  The two vocoder launches of rvcmi_glue_sola_pv_batch at S = 1, without an offset.         */
int rvcmi_glue_phase_vocoder(const float* a_dev, const float* b_dev, const float* fade_out_dev, const float* fade_in_dev, int n,
                             float* out_dev, double* scratch_dev, void* stream);

/* rvcmi_glue_sola with the GUI's use_pv branch (gui.py:1076-1087): the same search (first maximum), then
 * infer_wav[off : off + Lb] is cross-faded with sola_buffer by rvcmi_glue_phase_vocoder instead of the sin^2 fade; out_block_dev
 * and the new tail (sola_buffer_dev, in place) are cut from the result as in rvcmi_glue_sola, block_frame < Lb included.  The
 * offset stays on the device.  Lb <= 4096.  scratch_dev: 3 * (Lb/2 + 1) + Lb/2 + 1 doubles.
 * The bank form (rvcmi_glue_sola_pv_batch) at S = 1 with contiguous rows.                                                    */
int rvcmi_glue_sola_pv(const float* infer_wav_dev, int64_t n, float* sola_buffer_dev, int Lb, int Ls,
                       const float* fade_in_dev, const float* fade_out_dev, int block_frame, float* out_block_dev,
                       int* offset_out_dev, double* scratch_dev, void* stream);

/* The realtime GUI's envelope mix (gui.py:1023-1056), IN PLACE on wav_dev [n]:
 *   rms1, rms2 = frame RMS of input_dev[:n] and wav_dev (librosa.feature.rms, frame_length 4 zc, hop zc, centred, zero padded),
 *   both linearly interpolated with align_corners=True to n + 1 points, the last dropped;  rms2 = max(rms2, 1e-3);
 *   wav *= pow(rms1 / rms2, float32(1 - rate)).
 * scratch_dev: 2 * (1 + n / zc) floats.  Not the offline change_rms (half-second frames, align_corners=False, 1e-6).
 * The bank form (rvcmi_glue_envelope_mix_batch) at S = 1 with contiguous rows.                                                 */
int rvcmi_glue_envelope_mix(const float* input_dev, float* wav_dev, int64_t n, int zc, double rate, float* scratch_dev,
                            void* stream);

/* The realtime GUI's noise reduction (gui.py:869-871, 974-992, 1015-1022): TorchGate.forward(x, xn) of
 * infer/modules/gui/torchgate.py for B rows at once.  x_dev [B][n], xn_dev [B][nn] (NULL: the noise statistics come from x, the
 * reference's xn=None), all fp32; out_dev [B][hop * (n / hop)] fp32.  Per row:
 *   X = stft(x, n_fft, hop, window, center=True, zero padding, onesided);  X_db = amp_to_db(X) = max(20 log10(|X| + eps64), max_f - 40)
 *   stationary:      mask = X_db > mean_f(XN_db) + n_std_thresh * std_f(XN_db)   (unbiased std over the noise frames, per bin)
 *   non-stationary:  s = conv1d(|X|, ones(n_movemean), padding="same") / n_movemean over frames (xn unused);
 *                    mask = sigmoid(((|X| - s) / (s + 1e-6) - n_thresh_ns) / temp_coeff)
 *   mask = prop_decrease * (float(mask) - 1) + 1 (fp32);  filter_dev [nf][nt] fp32 (NULL: none): conv2d over (bin, frame),
 *   padding="same";  out = istft(X * mask): window * irfft, overlap-add, / sum of squared windows, n_fft / 2 trimmed at each end.
 * window_dev [n_fft] fp64 is torch.hann_window(win_length) zero-padded to the centre.  Spectra, dB, statistics, comparison and
 * overlap-add in fp64 (direct DFTs with exact (k m) mod n_fft twiddle reduction), one rounding at the end; the mask is fp32 like
 * the reference's.  n_fft even and <= 4096 (an odd n_fft, which torch accepts, is RVCMI_ERR_INVALID), 1 <= hop <= n_fft,
 * 0 <= prop_decrease <= 1.  Where the window envelope vanishes (torch.istft raises) the quotient is written as it falls.
 * Enqueue-only: no allocation, synchronisation or host read-back (graph-capturable); rows are independent, so a row's output
 * does not depend on B.  scratch_dev: rvcmi_glue_spectral_gate_scratch_bytes(B, n, xn_dev ? nn : 0, n_fft, hop) bytes.       */
int rvcmi_glue_spectral_gate(const float* x_dev, int B, int64_t n, const float* xn_dev, int64_t nn, int n_fft, int hop,
                             const double* window_dev, const float* filter_dev, int nf, int nt, int nonstationary,
                             double n_std_thresh, double n_thresh_ns, double temp_coeff, int n_movemean, double prop_decrease,
                             float* out_dev, void* scratch_dev, size_t scratch_bytes, void* stream);
/* Bytes of scratch rvcmi_glue_spectral_gate needs (nn = 0: no noise signal); 0 when the arguments are out of range. */
size_t rvcmi_glue_spectral_gate_scratch_bytes(int B, int64_t n, int64_t nn, int n_fft, int hop);

/* Where Pipeline.pipeline cuts a long input (infer/modules/vc/pipeline.py:219-236): for every t in range(t_center, n, t_center),
 *   cuts_dev[c] = t - t_query + first argmin of audio_sum[t - t_query : min(t + t_query, n)],
 *   audio_sum[j] = (((0 + |p[j]|) + |p[j + 1]|) + ... + |p[j + window - 1]|),  p = np.pad(audio, window / 2, mode="reflect"),
 * in IEEE fp64 with the adds in exactly that order, so the sums -- and the cuts -- are BIT-equal to numpy's `window` passes; only
 * the positions a search window looks at are computed.  audio_dev [n] fp64 (the filtfilt output); the reflection is index
 * arithmetic.  cuts_dev [>= len(range(t_center, n, t_center))] int64; sums_dev (or NULL) [cuts][2 t_query] fp64 receives the
 * window sums (entries past the end of the signal are left untouched).  RVCMI_ERR_INVALID, and nothing launched, when the number
 * of cuts exceeds max_cuts (or 65535), window is odd, below 2 or above 1024 (the LDS staging; the reference's is 160),
 * n <= window, or t_query > t_center (numpy's negative slice start would wrap there; no reference configuration has it).
 * Comparisons with NaN are false, so a NaN is never the minimum and a window of nothing but NaN yields its first position; the
 * reference raises IndexError as soon as a window holds one NaN (an enqueue-only call cannot raise on data).
 * Enqueue-only, deterministic (no float atomics).  scratch_dev: rvcmi_glue_cut_points_scratch_bytes(...) bytes.               */
int rvcmi_glue_cut_points(const double* audio_dev, int64_t n, int window, int64_t t_center, int64_t t_query, int64_t* cuts_dev,
                          int64_t max_cuts, double* sums_dev, void* scratch_dev, void* stream);
/* Bytes of scratch rvcmi_glue_cut_points needs; 0 when the arguments are out of range (or there is no cut). */
size_t rvcmi_glue_cut_points_scratch_bytes(int64_t n, int window, int64_t t_center, int64_t t_query);

/* scipy.signal.filtfilt(b, a, x) with scipy's defaults (padtype="odd", padlen = 3 * (order + 1), method="pad") for a ragged batch:
 * the input preparation of Pipeline.pipeline (infer/modules/vc/pipeline.py:23,221).  x_dev: one flat buffer of float (x_is_f64 = 0)
 * or double samples, widened on the device; offsets_dev [B + 1] int64 on the device, item i = x[offsets[i] .. offsets[i + 1]);
 * max_len (<= 2^28) >= the longest item and total >= offsets[B] are given by the host (they size the grid and the buffers; an item that
 * contradicts them, or is not longer than padlen, is left untouched).  b, a, zi are HOST arrays of order + 1, order + 1 and order
 * doubles, 1 <= order <= 8, a[0] == 1 (divide by a[0] first, as lfilter does), zi = lfilter_zi(b, a); they travel by value.
 * Both passes are direct form II transposed in fp64 with every operation rounded on its own (no FMA), each starting from
 * zi * first sample.  One thread produces 1024 consecutive outputs of a pass after a warm-up of `warmup` samples (a multiple of
 * 1024) that starts from zi * in[start]; no filter state is passed between threads.  The caller derives warmup from the poles so
 * that the start has decayed below 2^-64 (rvc_amd.glue.filt_warmup).  An item with n + 2 padlen <= warmup + 1024 is computed from
 * scipy's own initial state throughout and is BIT-equal to scipy; longer items differ from scipy by the rounding noise of an
 * independent fp64 evaluation of the recurrence.  Batch item i is computed exactly as a call with that item alone.
 * out_dev [total] fp64, same layout as x.  out_pad_dev (or NULL): item i's np.pad(out_i, pad, mode="reflect") at
 * offsets[i] + 2 pad i, n_i + 2 pad doubles (a copy, exact; written only for items with n_i > pad; pad < max_len).
 * The odd extension and the reversal of the second pass are index arithmetic.  Enqueue-only, no allocation, deterministic.
 * scratch_dev: rvcmi_glue_filtfilt_scratch_bytes(B, total, order) bytes (the forward pass's output).                          */
int rvcmi_glue_filtfilt(const void* x_dev, int x_is_f64, const int64_t* offsets_dev, int B, int64_t max_len, int64_t total,
                        const double* b, const double* a, const double* zi, int order, int warmup, double* out_dev, double* out_pad_dev,
                        int64_t pad, void* scratch_dev, size_t scratch_bytes, void* stream);
/* Bytes of scratch rvcmi_glue_filtfilt needs; 0 when the arguments are out of range. */
size_t rvcmi_glue_filtfilt_scratch_bytes(int B, int64_t total, int order);

/* The formant-shift resample of the realtime path (rtrvc.py:248-259, torchaudio.transforms.Resample(orig_freq = upp_res,
 * new_freq = tgt_sr / 100)): out[j * new + p] = sum_{k < K} kernel[p][k] * xpad[j * orig + k], xpad = x with `width` zeros in
 * front and zeros behind; orig / new already divided by their gcd; kernel_dev [new][K] (K = 2 * width + orig) is torchaudio's
 * windowed-sinc table (rvc_amd.realtime.sinc_resample_kernel restates its published formula: hann window, lowpass_filter_width 6,
 * rolloff 0.99).  n_out = ceil(new * n / orig) for the whole signal.  PARITY UNPINNED: torchaudio is not installable offline.
 * The bank form (rvcmi_glue_resample_poly_batch) at S = 1 with contiguous rows.                                               */
int rvcmi_glue_resample_poly(const float* x_dev, int64_t n, const float* kernel_dev, int orig, int new_, int K, int width,
                             float* out_dev, int64_t n_out, void* stream);

/* ---- the realtime block for a bank of S sessions (rvc_amd.RealtimeBank) ----------------------------------------------------
 * Each call below is its single-stream namesake applied to S signals at once: the same kernels and the same launch recipe (the
 * single-stream entry IS this one at S = 1), so session s's results equal a single-stream call on its row bit for bit, and the
 * number of launches does not depend on S.  Every per-session array is given with a ROW STRIDE in elements (`*_stride`): session s's row starts
 * at base + s * stride, and a row may be a slice of a longer rolling buffer (stride >= the row's length, else
 * RVCMI_ERR_INVALID).  Rows of one output array must not overlap.  1 <= S <= 65535.  Tables (resample kernel, fades) are shared. */

/* rvcmi_glue_resample_poly per row: x_dev rows of n samples -> out_dev rows of n_out samples. */
int rvcmi_glue_resample_poly_batch(int S, const float* x_dev, int64_t x_stride, int64_t n, const float* kernel_dev, int orig,
                                   int new_, int K, int width, float* out_dev, int64_t out_stride, int64_t n_out, void* stream);

/* rvcmi_glue_resample_poly_batch with a ratio PER ROW (the bank's formant shift per session, rtrvc.py:248-259): ONE launch, row s
 * resampled by its own descriptor rows_dev[s] -- its table kernels_dev + w_off ([new_][K], as rvcmi_glue_resample_poly takes it), its
 * reduced orig / new_, K, width, and the n <= n_max samples of the row it reads -- to n_out samples, bit-equal to
 * rvcmi_glue_resample_poly on that row with that table.  A row with orig == new_ is not resampled: its first n_out samples are copied
 * (zeros behind n).  kernels_dev holds kernels_floats floats, the tables of all distinct ratios back to back; a descriptor that points
 * outside it yields a row of zeros (the descriptors live on the device and are not read back).  x_stride < n_max, out_stride < n_out,
 * S < 1: RVCMI_ERR_INVALID. */
typedef struct {
    int64_t w_off;   /* first float of the row's table in kernels_dev */
    int64_t n;       /* input samples of the row                      */
    int orig, new_;  /* rates divided by their gcd                    */
    int K, width;    /* K = 2 * width + orig                          */
} rvcmi_resample_row;
int rvcmi_glue_resample_poly_ragged(int S, const float* x_dev, int64_t x_stride, int64_t n_max, const float* kernels_dev,
                                    int64_t kernels_floats, const rvcmi_resample_row* rows_dev, float* out_dev, int64_t out_stride,
                                    int64_t n_out, void* stream);

/* rvcmi_glue_sola per session: one offset search per session (one block each, the chunk head and the previous tail staged in
 * LDS: 2 Lb + Ls floats <= 150 KB), sola_buffer_dev [S rows of Lb] updated in place, out_block_dev [S rows of block_frame],
 * offset_out_dev [S] (optional, contiguous).                                                                              */
int rvcmi_glue_sola_batch(int S, const float* infer_wav_dev, int64_t wav_stride, int64_t n, float* sola_buffer_dev,
                          int64_t buf_stride, int Lb, int Ls, const float* fade_in_dev, const float* fade_out_dev,
                          int block_frame, float* out_block_dev, int64_t out_stride, int* offset_out_dev, void* stream);

/* rvcmi_glue_sola_pv per session (four launches for the whole bank).  Lb <= 4096.
 * scratch_dev: S * P doubles with P = 3 * (Lb/2 + 1) + Lb/2 + 1; session s owns [s * P, (s + 1) * P), laid out as the
 * single-stream call's scratch: bins [3 * (Lb/2 + 1)] doubles | phase-vocoder result [Lb] floats | the offset (one int, used
 * when offset_out_dev is NULL).                                                                                            */
int rvcmi_glue_sola_pv_batch(int S, const float* infer_wav_dev, int64_t wav_stride, int64_t n, float* sola_buffer_dev,
                             int64_t buf_stride, int Lb, int Ls, const float* fade_in_dev, const float* fade_out_dev,
                             int block_frame, float* out_block_dev, int64_t out_stride, int* offset_out_dev,
                             double* scratch_dev, void* stream);

/* rvcmi_glue_envelope_mix per session, IN PLACE on wav_dev rows of n samples against input_dev rows (their first n samples).
 * scratch_dev: S * 2 * (1 + n / zc) floats (per session: the input's envelope, then the output's).                         */
int rvcmi_glue_envelope_mix_batch(int S, const float* input_dev, int64_t in_stride, float* wav_dev, int64_t wav_stride,
                                  int64_t n, int zc, double rate, float* scratch_dev, void* stream);

/* rvcmi_glue_expand_protect per session (the bank without retrieval): feats_dev [S, nq, d], pitchf_dev [S, p_len] or NULL,
 * out_dev [S, p_len, d], contiguous.                                                                                       */
int rvcmi_glue_expand_protect_batch(int S, const float* feats_dev, int64_t nq, int d, int reps, const float* pitchf_dev,
                                    float protect, int64_t p_len, float* out_dev, void* stream);

/* The noise reduction of a bank (rvc_amd.TorchGateBank, RealtimeBank.set_noise_reduce): rvcmi_glue_spectral_gate, stationary with a
 * noise signal, for S sessions whose noise signal xn is a ROLLING buffer.  Between two calls every xn row moved left by `shift`
 * samples and its last `tail` samples were rewritten, so most of its Fn = 1 + nn / hop frames hold the samples of frame
 * f + shift / hop of the call before.  The caller keeps their spectra: ring_dev [S][Fn][K] double2 (K = n_fft / 2 + 1,
 * rvcmi_glue_spectral_gate_ring_bytes), logical frame f of THIS call in slot (ring_base + f) % Fn, so the caller adds shift / hop to
 * ring_base per call.  A frame is CLEAN -- kept, not transformed -- iff shift >= 0, shift % hop == 0, tail <= nn and
 *   shift > 0:   f hop - n_fft / 2 >= 0  and  f hop + n_fft / 2 <= nn - max(tail, shift);
 *   shift == 0:  tail == 0  or  f hop + n_fft / 2 <= nn - tail          (the frame keeps its slot, zero padding included);
 * anything else makes every frame dirty (the arithmetic of a cold call, not an error).  rvcmi_glue_gate_ring_plan is that rule.
 * mode_dev [S] uint8 on the device: 0 = the session is off: its out row, its ring rows and its scratch are not written;
 * 1 = warm: only the dirty frames are transformed and stored (the caller vouches that the session's ring rows hold the previous
 * call's spectra under the previous ring_base); 2 = cold: all Fn frames are.  any_cold (host): non-zero when some session is cold;
 * the launch covers all noise tiles only then (a cold session with any_cold = 0 would be left with stale rows).  Blocks of off
 * sessions and of a warm session's surplus tiles leave on a branch that is uniform per block.
 * BIT-EQUALITY: a frame's spectrum is summed in an order that depends on neither its place in a tile nor its slot, and the
 * statistics pass reads the cache in logical frame order, so every active session's out row is bit-equal to rvcmi_glue_spectral_gate
 * on contiguous copies of its x and xn rows -- warm or cold, whatever S and whatever the other sessions do.  The launch count (six)
 * does not depend on S.  x_dev rows of n, xn_dev rows of nn, out_dev rows of hop * (n / hop) samples, each with its row stride.
 * out_dev MAY ALIAS x_dev (same rows): the overlap-add reads only scratch.  It must not overlap xn_dev.  nonstationary must be 0
 * (the non-stationary mask ignores xn): RVCMI_ERR_INVALID, as are S outside 1 .. 65535, a stride shorter than its row, an odd n_fft
 * or one above 4096, and a ring or scratch smaller than the _bytes functions say.  Enqueue-only, no allocation.                  */
int rvcmi_glue_spectral_gate_ring_batch(int S, const float* x_dev, int64_t x_stride, int64_t n, const float* xn_dev, int64_t xn_stride,
                                        int64_t nn, float* out_dev, int64_t out_stride, int64_t shift, int64_t tail, void* ring_dev,
                                        size_t ring_bytes, int64_t ring_base, const uint8_t* mode_dev, int any_cold, int n_fft, int hop,
                                        const double* window_dev, const float* filter_dev, int nf, int nt, int nonstationary,
                                        double n_std_thresh, double prop_decrease, void* scratch_dev, size_t scratch_bytes, void* stream);
/* Bytes of scratch / of the spectrum cache the call above needs; 0 when the arguments are out of range. */
size_t rvcmi_glue_spectral_gate_ring_scratch_bytes(int S, int64_t n, int n_fft, int hop);
size_t rvcmi_glue_spectral_gate_ring_bytes(int S, int64_t nn, int n_fft, int hop);
/* The dirty-frame rule on the host (no device needed): plan_out[6] = { Fn, K, head, back, advance, n_dirty }: the dirty frames are
 * [0, head) and [back, Fn) (head == back == Fn: all of them), advance = shift / hop is what the caller adds to ring_base before the
 * call (0 when every frame is dirty).  RVCMI_ERR_INVALID when nn < 1, n_fft is odd or outside [2, 4096] or hop outside [1, n_fft]. */
int rvcmi_glue_gate_ring_plan(int64_t nn, int n_fft, int hop, int64_t shift, int64_t tail, int* plan_out);

/* The GUI's cross-fade of the gated input block (gui.py:986-990) for the sessions with mode_dev[s] != 0; g_dev rows of
 * block_frame + Lb samples (the gate's output), Lb <= block_frame:
 *   g[:Lb] = g[:Lb] * fade_in + nr_buffer * fade_out;   denoise[-block_frame:] = g[:block_frame];   nr_buffer = g[block_frame:]
 * with three fp32 roundings per faded sample and no fused multiply-add, so the result is bit-equal to torch's three element-wise
 * statements.  denoise_dev rows of den_len samples; den_prev_dev (or NULL: no roll) rows of den_len - block_frame samples, a COPY of
 * denoise[block_frame:] taken before the call, written to denoise[: den_len - block_frame] (the roll, per session: a session with
 * mode 0 keeps its row).  g_dev is not written.                                                                              */
int rvcmi_glue_nr_stitch_batch(int S, const float* g_dev, int64_t g_stride, int Lb, int64_t block_frame, const float* fade_in_dev,
                               const float* fade_out_dev, float* nr_buffer_dev, int64_t nr_stride, float* denoise_dev, int64_t den_stride,
                               int64_t den_len, const float* den_prev_dev, int64_t prev_stride, const uint8_t* mode_dev, void* stream);

/* Per session a copy chosen by mode_dev[s]: non-zero: dst[s][off_a : off_a + na] = a[s][:na]; zero: dst[s][off_b : off_b + nb] =
 * b[s][:nb], or nothing when b_dev is NULL.  dst_dev rows of dst_len samples.  A range that leaves its row: RVCMI_ERR_INVALID.     */
int rvcmi_glue_masked_write_batch(int S, float* dst_dev, int64_t dst_stride, int64_t dst_len, const float* a_dev, int64_t a_stride,
                                  int64_t off_a, int64_t na, const float* b_dev, int64_t b_stride, int64_t off_b, int64_t nb,
                                  const uint8_t* mode_dev, void* stream);

/* The realtime GUI's input gate (gui.py:950-963) per session, on the device: with x = rms_buffer | block (4 zc + blk samples),
 *   rms = librosa.feature.rms(x, frame_length 4 zc, hop zc)[2:]  (blk / zc + 3 centred frames, zero padded; the arithmetic of
 *         rvcmi_glue_envelope_mix's frame RMS: float32 squares, fp64 sum, the mean rounded to float32, sqrtf),
 *   frame i is quiet iff librosa.amplitude_to_db(rms)[i] < threhold,
 *   dst[j] = x[2 zc + j] for j < blk + 2 zc, zero iff frame (j + zc / 2) / zc (integer divisions) is quiet;  rms_buffer <- x[-4 zc:].
 * No logarithm is evaluated here: the decision is monotone in the float32 RMS, so the caller passes two float32 cutoffs derived on the
 * host from the threshold (rvc_amd.realtime.input_gate_cutoffs): quiet iff rms[i] < cut_a and max_i rms[i] < cut_b (the 80 dB clip under
 * the loudest frame); a NaN among the frames makes no frame quiet.
 * block_dev rows of blk samples, rms_buffer_dev rows of 4 zc (in / out), dst_dev rows of blk + 2 zc (the tail of a rolling buffer: a row
 * stride in elements each).  scratch_dev: S * rvcmi_glue_input_gate_scratch_floats(zc, blk) floats (per session the staged x, then its
 * frame RMS); x is read from there, never from a buffer being written.  Three launches whatever S.
 * RVCMI_ERR_INVALID: blk % zc != 0, blk < zc, zc < 1, S outside [1, 65535], a row stride shorter than its row.                        */
size_t rvcmi_glue_input_gate_scratch_floats(int zc, int blk);
int rvcmi_glue_input_gate_batch(int S, const float* block_dev, int64_t block_stride, float* rms_buffer_dev, int64_t rms_stride,
                                float* dst_dev, int64_t dst_stride, int zc, int blk, float cut_a, float cut_b, float* scratch_dev,
                                void* stream);

/* rvcmi_glue_envelope_mix_batch and rvcmi_glue_input_gate_batch with their control PER SESSION (the GUI's rms_mix_rate and threhold sliders, gui.py:1024-1056, 950-963), for a
 * bank whose talkers move them independently.  The values are given twice, as rvcmi_glue_rmvpe_f0_ragged takes its rows: sess_host is
 * checked before anything is launched, sess_dev (the same bytes in device memory) is what the kernels read.  The kernels call the
 * device bodies of the _batch kernels, so an active session's arithmetic is the same instructions in the same order; the blocks of
 * an inactive session leave on a branch that is uniform per block.  Enqueue-only, no allocation; the launch count (three) depends on
 * neither S nor on which sessions are active (with none active: rvcmi_glue_envelope_mix_sessions launches nothing,
 * rvcmi_glue_input_gate_sessions its last kernel alone).  RVCMI_ERR_INVALID, nothing launched: S outside [1, 65535], an `on` that is
 * not 0 / 1, an exponent that is not finite, a cutoff that is negative or NaN, a row stride shorter than its row, and what the
 * _batch calls refuse.
 *
 * rvcmi_glue_envelope_mix_sessions: session s is mixed with the exponent sess[s].exponent = float32(1 - rate), computed on the host in
 * double and rounded once (as rvcmi_glue_envelope_mix_batch does with its scalar), iff sess[s].on; the wav row and the scratch of a
 * session that is off are not written.
 *
 * rvcmi_glue_input_gate_sessions: session s is gated with its own cutoffs iff sess[s].on.  A session that is off (threhold <= -60)
 * ends as the stream that does not call the gate: the last blk samples of its dst row are the raw block, the 2 zc samples in front of
 * them and its rms_buffer row are not touched (the reference leaves the buffer stale while the slider is at or below -60).          */
typedef struct {
    float exponent;  /* float32(1 - rms_mix_rate) */
    int32_t on;      /* 0 / 1                     */
} rvcmi_session_mix;
typedef struct {
    float cut_a, cut_b;  /* rvc_amd.realtime.input_gate_cutoffs(the session's threhold) */
    int32_t on;          /* 0 / 1                                                       */
    int32_t reserved_;   /* 0                                                           */
} rvcmi_session_gate;
int rvcmi_glue_envelope_mix_sessions(int S, const float* input_dev, int64_t in_stride, float* wav_dev, int64_t wav_stride, int64_t n,
                                     int zc, const rvcmi_session_mix* sess_host, const rvcmi_session_mix* sess_dev, float* scratch_dev,
                                     void* stream);
int rvcmi_glue_input_gate_sessions(int S, const float* block_dev, int64_t block_stride, float* rms_buffer_dev, int64_t rms_stride,
                                   float* dst_dev, int64_t dst_stride, int zc, int blk, const rvcmi_session_gate* sess_host,
                                   const rvcmi_session_gate* sess_dev, float* scratch_dev, void* stream);

/* ---- beyond SURVEY.md section 8: the recurrent layer of the RMVPE f0 network -----------------------------------------------
 * Stands in for the `nn.GRU(384, 256, num_layers=1, batch_first=True, bidirectional=True)` of rvc/f0/e2e.py:50-67 (E2E.BiGRU, the
 * first module of E2E.fc), which bench.py --e2e measured at 75-90 % of a whole conversion on PyTorch-ROCm / MIOpen.
 * Weights in torch's layout and gate order (r, z, n), forward direction first: w_ih [2][3H][I], w_hh [2][3H][H], b_ih / b_hh [2][3H],
 * fp32 on the host.  hidden_size must be 256, input_size a multiple of 16 (anything else: RVCMI_ERR_INVALID, the caller keeps torch's).
 * Operands fp16 (x, W_ih, W_hh and the broadcast copy of h), accumulation / gates / state fp32.                                  */
typedef struct rvcmi_gru rvcmi_gru;
int rvcmi_gru_create(int input_size, int hidden_size, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                     int device, rvcmi_gru** out);
int rvcmi_gru_destroy(rvcmi_gru* h);
/* x16_dev [B][T][I] fp16; y_dev [B][T][2H] fp32 = nn.GRU's `output` with h_0 = 0; hn_dev [2][B][H] fp32 = its `h_n` (or NULL).
 * The projection workspace grows with the largest B * T seen (a hipMalloc on such a call: the FIRST call of a size must not be inside a
 * stream capture); the smaller workspaces it replaces stay allocated until destroy, so a graph captured earlier keeps replaying.
 * B outside 1 .. 65535, T < 1, B * T > 2^30: RVCMI_ERR_INVALID, nothing launched, the workspace untouched.                          */
int rvcmi_gru_forward(rvcmi_gru* h, int B, int T, const void* x16_dev, float* y_dev, float* hn_dev, void* stream);
/* The same for a RAGGED batch: nseq sequences packed along the row axis, sequence i in rows [offsets[i], offsets[i + 1]) of x16_dev [R][I]
 * and y_dev [R][2H], R = offsets[nseq]; hn_dev [2][nseq][H] or NULL.  offsets_host and offsets_dev hold the same nseq + 1 ints (the host
 * copy is checked, the device copy is what the kernel reads; the caller keeps both alive until the work has run).  Every sequence is
 * computed exactly as rvcmi_gru_forward(h, 1, its length, its rows) computes it, bit for bit: each direction starts from h_0 = 0 at the
 * sequence's own first / last row.  offsets[0] != 0, offsets that do not ascend strictly, nseq outside 1 .. 65535, R > 2^30:
 * RVCMI_ERR_INVALID, nothing launched.  The projection workspace grows with R as it does with B * T above.                        */
int rvcmi_gru_forward_ragged(rvcmi_gru* h, int nseq, const int* offsets_host, const int* offsets_dev, const void* x16_dev, float* y_dev,
                             float* hn_dev, void* stream);

/* ---- beyond SURVEY.md section 8: the deep U-Net of the RMVPE f0 network and its head -----------------------------------------
 * Stands in for `self.cnn(self.unet(mel))` of rvc/f0/e2e.py:46 (DeepUnet of rvc/f0/deepunet.py + Conv2d(16, 3, 3x3)): everything between
 * the transposed mel input and the GRU's input.  `weights`: fp32 host tensors under their state-dict names ("unet.encoder.bn.weight",
 * "unet.encoder.layers.0.conv.0.conv.0.weight", ..., "cnn.weight", "cnn.bias"; running statistics included, tensors with other prefixes
 * are ignored).  The geometry (levels, units per level, intermediate layers, base channels) is read from the names and shapes.  Supported:
 * one input channel, 128 mel bins, pooling (2, 2), channel counts that are multiples of 16; anything else, or a tensor under "unet." /
 * "cnn." the recognised network does not use: RVCMI_ERR_INVALID (the caller keeps torch's modules).  Operands and stored activations fp16,
 * accumulation and the BatchNorm / ReLU / residual epilogues fp32.  Results are bit-identical from run to run.                          */
typedef struct rvcmi_unet rvcmi_unet;
int rvcmi_unet_create(const rvcmi_tensor* weights, int n_weights, int device, rvcmi_unet** out);
int rvcmi_unet_destroy(rvcmi_unet* h);
int rvcmi_unet_head_channels(rvcmi_unet* h);
/* Bytes of device workspace one forward of (B, T) needs; 0 for a shape the handle does not serve (T not a multiple of 2^levels,
 * B * T > 2^22, a launch beyond the grid limits).                                                                                  */
size_t rvcmi_unet_workspace_bytes(rvcmi_unet* h, int B, int T);
/* Enqueue only.  mel_dev [B][T][128] fp32 (the [B, 1, T, 128] input of DeepUnet.forward); out_dev [B][T][head channels][128] fp32, i.e.
 * the `.transpose(1, 2).flatten(-2)` of e2e.py:46 already applied; ws_dev: rvcmi_unet_workspace_bytes(h, B, T) bytes, 256-byte aligned.
 * The handle allocates and frees nothing after create: safe inside a stream capture.                                                */
int rvcmi_unet_forward(rvcmi_unet* h, int B, int T, const float* mel_dev, float* out_dev, void* ws_dev, void* stream);
/* The same for a RAGGED batch: nseq sequences packed along the frame axis, sequence i in rows [offsets[i], offsets[i + 1]) of
 * mel_dev [R][128] and out_dev [R][head channels][128], R = offsets[nseq]; no row is spent on padding to the longest.  Every sequence sees
 * the zero border of its own convolutions at its first and last row -- the rows of its neighbours are never read -- so it comes out as
 * its own rvcmi_unet_forward(h, 1, its length, ...) gives it, up to the summation order of the layers that split their K loop (the split
 * is chosen from the launch size, R here).  offsets_host / offsets_dev: the same nseq + 1 ints on the host (checked) and on the device
 * (read by the kernels; both alive until the work has run).  nseq < 1, offsets[0] != 0, a length that is not a positive multiple of
 * 2^levels (so also offsets that do not ascend), R > 2^22, a launch beyond the grid limits: RVCMI_ERR_INVALID / 0 bytes, nothing launched.
 * Enqueue only, nothing allocated; ws_dev: rvcmi_unet_workspace_bytes_ragged bytes.                                                  */
size_t rvcmi_unet_workspace_bytes_ragged(rvcmi_unet* h, int nseq, const int* offsets_host);
int rvcmi_unet_forward_ragged(rvcmi_unet* h, int nseq, const int* offsets_host, const int* offsets_dev, const float* mel_dev,
                              float* out_dev, void* ws_dev, void* stream);
/* Test hook: ONE primitive on caller-supplied data (synchronous; allocates).  kind 0: 3x3 convolution, 1: 1x1, 2: transposed 3x3 stride 2,
 * 3: 2x2 average pool, 4 / 5: the one-input-channel 3x3 / 1x1 behind the input scale and shift (x0_dev fp32 [B][H][W]), 6: 3x3 with the
 * head's fp32 [B][H][Cout][W] output.  Activations fp16 [B][H][W][C]; w in torch's layout ([Cout][Cin][k][k]; kind 2: [Cin][Cout][3][3]);
 * out = relu?(acc * scale + shift) + res.  ksplit 0: the forward's own choice, else the number of K slices.                           */
int rvcmi_unet_debug_op(int kind, int B, int H, int W, int C0, int C1, int Cout, const float* w, const float* scale, const float* shift,
                        int relu, float in_scale, float in_shift, const void* x0_dev, const void* x1_dev, const void* res_dev,
                        void* out_dev, int ksplit, int device, void* stream);

/* ---- beyond SURVEY.md section 8: the log-mel front end and the head of the RMVPE f0 network ------------------------------------
 * With these two, rvcmi_unet_*, rvcmi_gru_* and rvcmi_glue_rmvpe_f0_key a C caller goes from a 16 kHz waveform to (pitch, pitchf):
 *   mel_forward [B][T_pad][128] -> unet_forward [B][T_pad][3][128] -> (fp16) gru_forward [B][T_pad][512] -> rmvpe_head [B * T_pad][360]
 *   -> glue_rmvpe_f0_key on the first T rows.
 *
 * rvcmi_mel: MelSpectrogram.forward(audio, keyshift=0, speed=1, center=True) of rvc/f0/mel.py:58-71 over rvc/f0/stft.py:165-180:
 *   reflect pad by n_fft / 2, periodic Hann window of win_length, magnitude of the one-sided transform, mel_basis @ magnitude,
 *   (round_half: rounded to fp16, where the reference's `.half()` sits), clamp(min=clamp), log (round_half: rounded to fp16 again, as
 *   torch's half log does); stored as fp32.  mel_basis_host [n_mels][n_fft / 2 + 1] fp32 is DATA: the reference's `mel_basis` buffer.
 *   Any matrix is served exactly (per row the sum runs over [first non-zero, last non-zero + 1)).  Transform, magnitude and mel sum
 *   are fp64.  Supported: n_fft == win_length == 1024, n_mels == 128, hop >= 1, clamp > 0; anything else RVCMI_ERR_INVALID (the
 *   caller keeps torch).                                                                                                        */
typedef struct rvcmi_mel rvcmi_mel;
int rvcmi_mel_create(int n_fft, int hop, int win_length, int n_mels, const float* mel_basis_host, float clamp, int device,
                     rvcmi_mel** out);
int rvcmi_mel_destroy(rvcmi_mel* h);
/* Frames of an n-sample input: n / hop + 1 (center=True); 0 when n <= n_fft / 2, which torch's reflection pad refuses. */
int64_t rvcmi_mel_frames(rvcmi_mel* h, int64_t n);
/* wav_dev [B][n] fp32 -> out_dev [B][T_pad][n_mels] fp32, T_pad >= T = rvcmi_mel_frames(h, n): the transposed [B, 1, T, 128] that
 * rvcmi_unet_forward reads (the transpose of e2e.py:44 is gone); frames T .. T_pad - 1 are written as zeros, the
 * F.pad(mel, (0, n_pad)) of rvc/f0/rmvpe.py:141-144.  Enqueue-only, allocates nothing (safe inside a stream capture), bit-identical
 * from run to run.  n <= n_fft / 2, T_pad < T, B outside 1 .. 65535: RVCMI_ERR_INVALID, nothing launched.                       */
int rvcmi_mel_forward(rvcmi_mel* h, int B, int64_t n, const float* wav_dev, int round_half, int T_pad, float* out_dev, void* stream);

/* Linear(512, 360) + sigmoid of rvc/f0/e2e.py:33-35 (the Dropout between them is the identity in eval), one launch on the current
 * device: salience[m][f] = sigmoid(sum_k y[m][k] * w[f][k] + b[f]).  y_dev [M][512] (the GRU's output), w_dev [360][512], b_dev [360],
 * all fp32 on the device and 16-byte aligned; operands rounded to fp16 when half_operands, else fp32; fp32 MFMA accumulation over K in
 * chunks of 32 whose sums, the bias and the sigmoid are carried in fp64 and rounded once to fp32.  salience_dev [M][360] fp32.     */
int rvcmi_rmvpe_head(const float* y_dev, int M, const float* w_dev, const float* b_dev, int half_operands, float* salience_dev,
                     void* stream);

/* ---- beyond SURVEY.md section 8: HuBERT's convolutional feature extractor -------------------------------------------------------
 * Stands in for the `feature_extractor` of a HuBERT-base content encoder (fairseq ConvFeatureExtractionModel with extractor_mode
 * "default"; transformers HubertFeatureEncoder with feat_extract_norm "group"): seven bias-free Conv1d layers, 1 -> 512 k 10 stride 5 with
 * GroupNorm(512 groups, eps 1e-5, affine), 512 -> 512 k 3 stride 2 four times, 512 -> 512 k 2 stride 2 twice, exact (erf) GELU after each.
 * `weights`: fp32 host tensors under fairseq's names, "conv_layers.<i>.0.weight" ([512][1][10], [512][512][3], [512][512][2]) and
 * "conv_layers.0.2.weight" / ".bias" ([512]).  A missing tensor: RVCMI_ERR_MISSING; another shape, or any further tensor (a conv bias, an
 * eighth layer): RVCMI_ERR_INVALID (the caller keeps torch's module).  Operands and inter-layer streams fp16, accumulation and epilogues
 * fp32, the GroupNorm statistics fp64 from the centred covariance of the input.  Results are bit-identical from run to run.          */
typedef struct rvcmi_hubert_fe rvcmi_hubert_fe;
int rvcmi_hubert_fe_create(const rvcmi_tensor* weights, int n_weights, int device, rvcmi_hubert_fe** out);
int rvcmi_hubert_fe_destroy(rvcmi_hubert_fe* h);
/* Output frames of an N-sample input: (N - 400) / 320 + 1; 0 when N < 400 or N > 2^30. */
int64_t rvcmi_hubert_fe_frames(int64_t N);
/* Bytes of device workspace one forward of (B, N) needs; 0 for a shape that is not served (B outside 1 .. 65535, N outside 400 .. 2^30). */
size_t rvcmi_hubert_fe_workspace_bytes(rvcmi_hubert_fe* h, int B, int64_t N);
/* Enqueue only.  x_dev [B][N] fp16 (x_is_half) or fp32; out16_dev [B][frames][512] fp16, channels-last (the caller views it as
 * [B, 512, frames]).  ws_dev: rvcmi_hubert_fe_workspace_bytes(h, B, N) bytes, 256-byte aligned -- the handle then allocates nothing (safe
 * inside a stream capture); or NULL: the handle's own workspace, which grows with the largest shape seen (a hipMalloc on such a call: the
 * FIRST call of a size must not be inside a stream capture) while the smaller ones it replaces stay allocated until destroy, so a graph
 * captured earlier keeps replaying.  A shape that is not served: RVCMI_ERR_INVALID, nothing launched, the workspace untouched.
 * (For the tests: the workspace begins with layer 0's output, fp16 [B][L0][512], L0 = (N - 10) / 5 + 1; layers 2 and 4 reuse that buffer
 * from its start, so with B == 1 the rows from layer 2's count on still hold layer 0 after the forward.)                              */
int rvcmi_hubert_fe_forward(rvcmi_hubert_fe* h, int B, int64_t N, const void* x_dev, int x_is_half, void* out16_dev, void* ws_dev,
                            void* stream);
/* A RAGGED batch: x_dev [B][N_max], item i = its first lens[i] samples; what lies behind them is never read for a valid output and may be
 * anything (NaN included).  out16_dev [B][frames(N_max)][512] fp16: rows t < frames(lens[i]) of item i are BIT-equal to
 * rvcmi_hubert_fe_forward(h, 1, lens[i], ...) on that item alone (its statistics chunks and their merge order depend on its own length only,
 * a GEMM output row on no other row of its tile); the rows behind them are exactly zero.  lens_host / lens_dev: the same B ints on the host
 * (checked) and on the device (read by the kernels, also on every replay of a capture).  Workspace and capture rules as for the dense entry;
 * the bytes are those of the dense (B, N_max).  B outside 1 .. 65535, a lens[i] outside 400 .. N_max, N_max > 2^30, no item as long as N_max,
 * or a null lens pointer: RVCMI_ERR_INVALID, nothing launched.  Tiles wholly behind an item's end return at once, so the time follows the
 * sum of the lengths rather than B * N_max.                                                                                              */
size_t rvcmi_hubert_fe_workspace_bytes_ragged(rvcmi_hubert_fe* h, int B, int64_t N_max);
int rvcmi_hubert_fe_forward_ragged(rvcmi_hubert_fe* h, int B, int64_t N_max, const int* lens_host, const int* lens_dev, const void* x_dev,
                                   int x_is_half, void* out16_dev, void* ws_dev, void* stream);
/* Test hook: ONE of layers 1 - 6 WITHOUT the activation on caller-supplied data (synchronous; allocates).  taps 3 or 2; w in torch's layout
 * [512][512][taps] on the host; x16_dev fp16 [B][L_in][512]; out32_dev fp32 [B][(L_in - taps) / 2 + 1][512].                          */
int rvcmi_hubert_fe_debug_conv(int taps, int B, int L_in, const float* w, const void* x16_dev, float* out32_dev, int device, void* stream);

/* ---- beyond SURVEY.md section 8: HuBERT's transformer encoder layers -------------------------------------------------------------
 * The repeated block of a post-norm HuBERT (fairseq TransformerSentenceEncoderLayer with layer_norm_first = False; transformers
 * HubertEncoderLayer): x = LN(x + Attn(x)); x = LN(x + FFN(x)), exact (erf) GELU, q scaled by head_dim^-0.5 after its bias.  Served: head
 * dim 64 (heads * 64 == d), d a multiple of 64 up to 1024, ffn a multiple of 64 up to 4096, 1 .. 64 layers, 0 < ln_eps < 1; anything else
 * RVCMI_ERR_INVALID (the caller keeps torch's modules).  `weights`: fp32 host tensors under fairseq's names, for every layer i
 * "layers.<i>.self_attn.{q,k,v,out}_proj.{weight,bias}", "layers.<i>.self_attn_layer_norm.*", "layers.<i>.fc1.*", "layers.<i>.fc2.*",
 * "layers.<i>.final_layer_norm.*" (Linear weights [out][in]).  A missing tensor: RVCMI_ERR_MISSING; another shape or any further tensor:
 * RVCMI_ERR_INVALID.  MFMA operands fp16 (weights, the layer's input, q / k / v, the probabilities, the attention output, the stream in
 * front of FFN-1, the GELU output), accumulation, softmax, residual adds and LayerNorm statistics fp32.  Five launches per layer; results
 * are bit-identical from run to run, and an item's rows do not depend on the other items of the batch.                                  */
typedef struct rvcmi_hubert_enc rvcmi_hubert_enc;
int rvcmi_hubert_enc_create(const rvcmi_tensor* weights, int n_weights, int n_layers, int d, int heads, int ffn, float ln_eps, int device,
                            rvcmi_hubert_enc** out);
int rvcmi_hubert_enc_destroy(rvcmi_hubert_enc* h);
/* Bytes of device workspace a forward of (B, T) needs; 0 for a shape that is not served (B outside 1 .. 65535, T < 1, B * T > 2^22). */
size_t rvcmi_hubert_enc_workspace_bytes(rvcmi_hubert_enc* h, int B, int T);
/* Enqueue only: layers first_layer .. first_layer + n - 1.  x_dev / out_dev [B][T][d], rows contiguous, fp16 (is_half) or fp32, 16-byte
 * aligned; every layer's output is rounded once to that dtype, so n layers in one call are BIT-equal to n calls of one layer.
 * key_mask_dev: uint8 [B][T] on the device, 1 = a padded key (its score is -inf), or NULL; padded QUERY rows are computed like any other.
 * ws_dev: the caller's, rvcmi_hubert_enc_workspace_bytes(h, B, T) bytes, 256-byte aligned; the handle allocates nothing here (safe inside a
 * stream capture).  A null pointer, a layer range outside the handle's, a shape that is not served: RVCMI_ERR_INVALID, nothing launched.
 * (For the tests: the workspace holds, each 256-byte aligned and in this order, q / k / v fp16 [3][B][heads][T][64], the attention output fp16
 * [B T][d], the stream behind the first LayerNorm fp32 [B T][d] and again fp16, then the GELU output fp16 [B T][ffn] of the LAST layer run.) */
int rvcmi_hubert_enc_forward(rvcmi_hubert_enc* h, int first_layer, int n, int B, int T, const void* x_dev, int is_half,
                             const uint8_t* key_mask_dev, void* out_dev, void* ws_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RVCMI_H */
