// IVF-Flat (faiss IndexIVFFlat, METRIC_L2) retrieval for gfx950: nearest-centroid probe, in-list
// squared-L2 scan with a per-wave top-k, and the reference's inverse-square blend
// (infer/modules/vc/pipeline.py:126-138, infer/lib/rtrvc.py:172-185; index recipe web.py:544-563).
//
// This half of the hot path is HBM/L2-bound byte movement (a few dozen 1-3 KB rows per query), so it
// is written as coalesced 16-byte row reads + wavefront-level reductions, NOT reshaped into a GEMM.
// Distances are evaluated in fp64 on the fp32 inputs as sum((q-v)^2) -- the arithmetic cost is
// irrelevant next to the row traffic, and it makes the ranking independent of summation order, which
// is what allows bit-exact indices against the CPU oracle (ties -> lowest id).
//
// Layout of the unit: the kernels are in ivf_kernels.hpp (coarse quantiser, query-major scan, blend, k-means helpers),
// ivf_lm_kernels.hpp (list-major scan) and ivf_add_kernels.hpp (device-side add); the device blob and faiss' file format are the
// host-only ivf_format.hpp, the host steps of k-means ivf_kmeans.hpp.  Here: the handle, the search workspace and routing, the
// launches, and the C ABI.
#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "common.hpp"
#include "ivf_format.hpp"
#include "ivf_kmeans.hpp"
#include "ivf_kernels.hpp"
#include "ivf_lm_kernels.hpp"
#include "ivf_add_kernels.hpp"
#include "session_rows.hpp"

using namespace rvcmi;

struct rvcmi_ivf {
    int device = 0;
    BlobHeader hdr;
    char* blob = nullptr;  // device
    bool owns_blob = false;
    // search workspace (grown on demand; see rvcmi_ivf_reserve)
    int64_t cap_nq = 0;
    int cap_nprobe = 0;
    DevBuf assign, P, Dtmp, Itmp, flag, cdist, cscore, qcnt, qperm;
    DevBuf bank_q, bank_flags;  // rvcmi_ivf_search_blend_expand_batch: the sessions' searched rows packed for one search, and flags [S]
    int64_t bank_cap_rows = 0, bank_cap_S = 0;
    int64_t cap_chunk = 0;  // queries per coarse-score chunk (bounds the nq x nlist fp32 scratch)
    // list-major scan (ivf_lm_kernels.hpp): row norms + statistics (once per handle), score scratch and work items (per capacity)
    DevBuf lm_rn, lm_S, lm_items, lm_n, lm_qinfo;
    bool lm_ready = false;
    double lm_vmax = 0.0;      // max |v| over the stored rows (error bound of the fp32 prefilter)
    int64_t lm_maxlen = 0;     // longest list
    int64_t lm_cap_items = 0;  // capacity of lm_items
    int64_t lm_cap_nq = 0;     // queries a call may bring for the list-major kernels (0: not reserved -- they never run)
    int64_t lm_buf_nq = 0;     // queries lm_S / lm_qinfo / lm_items are sized for = one PASS: a larger call runs several (the score scratch,
                               // queries x longest list x 4 B, is kept at or below 1 GiB)
    bool lm_warned = false;    // the one-time "large call on the query-major scan" diagnostic was printed
    Profiler prof;
    // dev / test options (common.hpp Options): IVF_COARSE_F64 (brute-force fp64 coarse quantizer), IVF_GENERIC (any-d scan kernel),
    // IVF_STAMPS (prints; syncs), IVF_DBG, IVF_SORT (1 = scan the queries in list-sorted, XCD-contiguous order).  Read from RVCMI_<KEY> once at handle creation; later only rvcmi_ivf_set_option.
    rvcmi::Options opt;
    rvcmi_ivf() { opt.load_env({"IVF_COARSE_F64", "IVF_GENERIC", "IVF_STAMPS", "IVF_DBG", "IVF_SORT", "IVF_LM", "IVF_LM_MIN"}); }
    const float* centroids() const { return (const float*)(blob + hdr.off_centroids); }
    const float4* centroids_t() const { return (const float4*)(blob + hdr.off_centroids_t); }
    const float* cnorm() const { return (const float*)(blob + hdr.off_cnorm); }
    const int64_t* list_off() const { return (const int64_t*)(blob + hdr.off_list_offsets); }
    const int64_t* ids() const { return (const int64_t*)(blob + hdr.off_ids); }
    const float* vecs() const { return (const float*)(blob + hdr.off_vecs); }
    ~rvcmi_ivf() {
        if (owns_blob && blob) (void)hipFree(blob);
    }
};

namespace rvcmi {

static rvcmi_ivf* from_host_blob(const std::vector<char>& blob, int device) {
    DeviceGuard dg(device);
    std::unique_ptr<rvcmi_ivf> h(new rvcmi_ivf());
    h->device = device;
    memcpy(&h->hdr, blob.data(), sizeof(BlobHeader));
    HIP_CHECK(hipMalloc((void**)&h->blob, blob.size()));
    h->owns_blob = true;
    HIP_CHECK(hipMemcpy(h->blob, blob.data(), blob.size(), hipMemcpyHostToDevice));
    return h.release();
}

// faiss.read_index: parsed and laid out on the host (ivf_format.hpp); a file that is refused never reaches the device
static rvcmi_ivf* read_faiss(const char* path, int device) { return from_host_blob(parse_faiss(path).blob(), device); }

static void write_faiss(const rvcmi_ivf* h, const char* path) {
    std::vector<char> blob(h->hdr.total_bytes);
    HIP_CHECK(hipMemcpy(blob.data(), h->blob, blob.size(), hipMemcpyDeviceToHost));
    write_faiss(blob, path);
}

// List-major scan: usable for nprobe 1, d a multiple of the MFMA K chunk, a list count the planner holds in LDS, and a score scratch
// (nq x longest list, fp32) of at most 1 GiB; fewer than 16 queries keep the one-launch query-major kernel.  (A list longer than the
// 2048-entry LDS row of the selector is worked on in place in the global scratch, round 5.)  Option IVF_LM: 0 = never, default 1.
// Returns nullptr when the list-major kernels can take a call of nq queries, else the reason they cannot (printed once per handle
// for calls of 64 queries or more: such a call silently costs the 34x row re-reads of the query-major scan otherwise).
static const char* lm_unusable_reason(const rvcmi_ivf* h, int64_t nq) {
    const BlobHeader& b = h->hdr;
    // from 16 queries on (round 5; 64 before): a realtime chunk's 16 guarded rows take 8 + 11 + 13 us in plan + tiles + select against 51 us in
    // the query-major kernel, whose one block per query walks a ~300-row list alone (chunk p50 0.487 -> 0.465 ms, ABAB); option IVF_LM_MIN
    const int lm_min = h->opt.geti("IVF_LM_MIN", 16);
    if (nq < lm_min) {
        static thread_local char why[64];
        snprintf(why, sizeof(why), "fewer than %d queries%s", lm_min, lm_min == 16 ? "" : " (option IVF_LM_MIN)");
        return why;
    }
    if (std::min<int64_t>(b.nprobe, b.nlist) != 1) return "nprobe > 1";
    if ((b.d % CG_K) != 0) return "d is not a multiple of 32";
    if (b.nlist > LM_MAXL) return "more than 16384 lists (the one-block planner counts them in LDS)";
    if (b.ntotal < 1) return "empty index";
    if (!h->lm_ready || h->lm_maxlen < 1) return "list statistics not reserved";
    if (nq >= (1ll << 30)) return "2^30 queries or more";
    // a pass holds at least 64 queries (lm_pass_queries): with one list of more than 2^22 rows even that pass would exceed the 1 GiB bound of
    // the score scratch (the bound was documented but the 64-query floor could break it by a wide margin)
    if ((int64_t)align_up((uint64_t)h->lm_maxlen, 32) * 4 * 64 > ((int64_t)1 << 30))
        return "a list of more than 4 194 304 rows (64 queries x the longest list x 4 B would exceed the 1 GiB score scratch)";
    return nullptr;
}
// queries per pass of the list-major kernels: the fp32 score scratch (queries x longest list) stays at or below 1 GiB
static int64_t lm_pass_queries(const rvcmi_ivf* h) {
    const int64_t pitch = (int64_t)align_up((uint64_t)std::max<int64_t>(h->lm_maxlen, 1), 32);
    return std::max<int64_t>(64, ((int64_t)1 << 30) / (pitch * 4));
}
static bool lm_usable(const rvcmi_ivf* h, int64_t nq) { return lm_unusable_reason(h, nq) == nullptr; }
static void lm_reserve(rvcmi_ivf* h, int64_t nq) {
    const BlobHeader& b = h->hdr;
    if (std::min<int64_t>(b.nprobe, b.nlist) != 1 || (b.d % CG_K) != 0 || b.nlist > LM_MAXL || b.ntotal < 1) return;
    if (!h->lm_ready) {  // once per handle (never inside a stream capture: reserve() runs before the first search)
        h->lm_rn.alloc((size_t)b.ntotal * 4);
        h->lm_n.alloc(256);
        HIP_CHECK(hipMemset(h->lm_n.p, 0, 256));
        hipLaunchKernelGGL(k_lm_row_norms, dim3((unsigned)((b.ntotal + 3) / 4)), dim3(256), 0, nullptr, h->vecs(), b.ntotal, b.d, h->lm_rn.as<float>());
        const int64_t m = std::max<int64_t>(b.ntotal, b.nlist);
        hipLaunchKernelGGL(k_lm_stats, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, nullptr, h->lm_rn.as<float>(), b.ntotal, h->list_off(), b.nlist,
                           h->lm_n.as<unsigned>() + 16);
        HIP_CHECK(hipGetLastError());
        unsigned st2[2];
        HIP_CHECK(hipMemcpy(st2, h->lm_n.as<unsigned>() + 16, 8, hipMemcpyDeviceToHost));
        float vm2;
        memcpy(&vm2, &st2[0], 4);
        h->lm_vmax = std::sqrt((double)vm2) * (1.0 + 1e-6);  // (the norms are fp32-rounded: a hair of head room)
        h->lm_maxlen = (int64_t)st2[1];
        static std::atomic<unsigned long long> attr_done{0};
        const unsigned long long bit = 1ull << (h->device & 63);
        if (!(attr_done.load() & bit)) {
            HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lm_plan), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (LM_MAXL + 1) * 4));
            attr_done.fetch_or(bit);
        }
        h->lm_ready = true;
    }
    // (declining to allocate must also retire an earlier, smaller reservation: reserve() raises cap_nq to the new value, and a later
    //  search with nq <= cap_nq would otherwise run the list-major kernels on buffers sized for fewer queries)
    h->lm_cap_nq = h->lm_buf_nq = 0;
    if (!lm_usable(h, std::max<int64_t>(nq, 64))) return;  // (option IVF_LM_MIN lowers only the routing threshold)
    const int64_t pitch = (int64_t)align_up((uint64_t)h->lm_maxlen, 32);
    const int64_t nb = std::min<int64_t>(std::max<int64_t>(nq, 1), lm_pass_queries(h));  // queries of one pass
    h->lm_S.alloc((size_t)nb * pitch * 4);
    h->lm_qinfo.alloc((size_t)nb * sizeof(LmQuery));
    // worst case of the planner: every probed list adds at most one partial query tile on top of nb / 32 full ones
    h->lm_cap_items = (nb / 32 + std::min<int64_t>(nb, b.nlist) + 1) * (pitch / 32);
    h->lm_items.alloc((size_t)h->lm_cap_items * sizeof(LmItem));
    h->lm_buf_nq = nb;
    h->lm_cap_nq = std::max<int64_t>(nq, 1);
}

static void reserve(rvcmi_ivf* h, int64_t nq) {
    const int np = (int)std::min<int64_t>(h->hdr.nprobe, h->hdr.nlist);
    const bool have_scores = np > 1 || (h->cscore.p && h->cap_chunk > 0);
    if (nq <= h->cap_nq && np <= h->cap_nprobe && h->flag.p && have_scores) {
        // the list-major scratch has a capacity of its own: a reserve above its 1 GiB bound retires it (lm_reserve), a later call
        // that fits gets it back at its own size
        if (h->lm_ready && nq > h->lm_cap_nq && lm_usable(h, nq)) {
            DeviceGuard dg(h->device);
            lm_reserve(h, nq);
        }
        return;
    }
    DeviceGuard dg(h->device);
    nq = std::max<int64_t>(nq, h->cap_nq);
    h->assign.alloc((size_t)std::max<int64_t>(nq, 1) * np * 8);
    h->P.alloc((size_t)std::max<int64_t>(nq, 1) * KMAX * 8);
    h->Dtmp.alloc((size_t)std::max<int64_t>(nq, 1) * KMAX * 4);
    h->Itmp.alloc((size_t)std::max<int64_t>(nq, 1) * KMAX * 8);
    if (!h->flag.p) h->flag.alloc(256);
    h->qcnt.alloc((size_t)(h->hdr.nlist + 1) * 4);
    h->qperm.alloc((size_t)std::max<int64_t>(nq, 1) * 4);
    if (np > 1) h->cdist.alloc((size_t)std::max<int64_t>(nq, 1) * h->hdr.nlist * 8);
    else {
        const int64_t per = std::max<int64_t>(64, (int64_t)(512ll << 20) / (h->hdr.nlist * 4));  // <= 512 MiB of scores
        h->cap_chunk = std::min<int64_t>(std::max<int64_t>(nq, 1), per);
        h->cscore.alloc((size_t)h->cap_chunk * h->hdr.nlist * 4);
    }
    h->cap_nq = nq;
    h->cap_nprobe = np;
    lm_reserve(h, nq);
}

struct BlendFuse {
    float* feats;
    float rate, omr;
};
// returns true when the blend of `bf` was done inside the scan kernel
static bool search(rvcmi_ivf* h, int64_t nq, const float* q, int k, float* D, int64_t* I, hipStream_t st,
                   const BlendFuse* bf = nullptr) {
    if (!h || nq < 0 || (nq && (!q || !D || !I))) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
    if (k < 1 || k > KMAX)
        RVCMI_FAIL(RVCMI_ERR_INVALID, "k=%d outside [1,%d]: the kernels keep at most %d neighbours per query (RVC asks for 8, "
                   "pipeline.py:126; legacy top-1 tools/cmd/infer-pm-index256.py:161)", k, KMAX, KMAX);
    if (nq == 0) return false;
    DeviceGuard dg(h->device);  // a C caller's current device need not be the handle's (restored on return)
    reserve(h, nq);
    const BlobHeader& b = h->hdr;
    const int d = b.d;
    const int np = (int)std::min<int64_t>(b.nprobe, b.nlist);
    HIP_CHECK(hipMemsetAsync(h->flag.p, 0, 4, st));
    const double cflops = 3.0 * (double)nq * b.nlist * d;
    if (np == 1 && !h->opt.on("IVF_COARSE_F64")) {
        // fp32 MFMA prefilter + fp64 verification (exactly the fp64 argmin; see k_coarse_pick)
        h->prof.launch("ivf_coarse", 2.0 * (double)nq * b.nlist * d, (double)nq * d * 4 + (double)b.nlist * d * 4 + 2.0 * nq * b.nlist * 4, st, [&] {
            if (h->cap_chunk <= 0 || !h->cscore.p) RVCMI_FAIL(RVCMI_ERR_INVALID, "coarse score scratch not reserved");
            for (int64_t qs = 0; qs < nq; qs += h->cap_chunk) {
                const int64_t nqc = std::min<int64_t>(h->cap_chunk, nq - qs);
                const int64_t big_blocks = ((b.nlist + 127) / 128) * ((nqc + 63) / 64);
                if (big_blocks >= 512) {
                    dim3 grid((unsigned)((b.nlist + 127) / 128), (unsigned)((nqc + 63) / 64));
                    hipLaunchKernelGGL((k_coarse_gemm<2, 4>), grid, dim3(256), 0, st, q + qs * d, h->centroids(), h->cnorm(), nqc,
                                       b.nlist, d, h->cscore.as<float>());
                } else {
                    dim3 grid((unsigned)((b.nlist + 31) / 32), (unsigned)((nqc + 31) / 32));
                    hipLaunchKernelGGL(k_coarse_gemm_ks, grid, dim3(256), 0, st, q + qs * d, h->centroids(), h->cnorm(), nqc,
                                       b.nlist, d, h->cscore.as<float>());
                }
                hipLaunchKernelGGL(k_coarse_pick, dim3((unsigned)((nqc + 3) / 4)), dim3(256), 0, st, q + qs * d, h->centroids(),
                                   h->cscore.as<float>(), nqc, b.nlist, d, b.cmax, h->assign.as<int64_t>() + qs);
            }
        });
    } else if (np == 1) {
        const size_t smem = align_up((size_t)QT * d * 4, 16) + 4 * QT * 16;
        h->prof.launch("ivf_coarse", cflops, (double)nq * d * 4 + (double)b.nlist * d * 4, st, [&] {
            hipLaunchKernelGGL(k_coarse1, dim3((unsigned)((nq + QT - 1) / QT)), dim3(256), smem, st, q, h->centroids_t(), nq,
                               b.nlist, d, h->assign.as<int64_t>());
        });
    } else {
        h->prof.launch("ivf_coarse", cflops, (double)nq * b.nlist * 8, st, [&] {
            const int64_t tot = nq * b.nlist;
            hipLaunchKernelGGL(k_coarse_dist, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, q, h->centroids(), nq,
                               b.nlist, d, h->cdist.as<double>());
            hipLaunchKernelGGL(k_coarse_select, dim3((unsigned)nq), dim3(64), 0, st, h->cdist.as<double>(), b.nlist, np,
                               h->assign.as<int64_t>());
        });
    }
    // list-major scan: plan (sort + work items) -> fp32 MFMA score tiles -> per-query exact verification (+ fused blend)
    const bool lm_wanted = h->opt.geti("IVF_LM", 1) && !h->opt.on("IVF_GENERIC");
    if (lm_wanted && nq >= 64 && !h->lm_warned) {
        const char* why = lm_unusable_reason(h, nq);
        if (why) {
            h->lm_warned = true;
            fprintf(stderr, "[rvcmi] ivf search: %lld queries run on the query-major scan (every probed list is re-read per query) because the "
                    "list-major kernels do not take this call: %s.  Printed once per index.\n", (long long)nq, why);
        }
    }
    if (lm_wanted && lm_usable(h, nq) && h->lm_S.p && nq <= h->lm_cap_nq && h->lm_buf_nq > 0) {
        const int pitch = (int)align_up((uint64_t)h->lm_maxlen, 32);
        const double rows = (double)b.ntotal / (double)b.nlist;
        // passes of at most lm_buf_nq queries (one, unless queries x longest list x 4 B would exceed the 1 GiB score scratch)
        for (int64_t qs = 0; qs < nq; qs += h->lm_buf_nq) {
            const int64_t nqp = std::min<int64_t>(h->lm_buf_nq, nq - qs);
            const float* qp = q + qs * d;
            const int64_t* asg = h->assign.as<int64_t>() + qs;
            h->prof.launch("ivf_plan", 0.0, (double)nqp * 12 + (double)b.nlist * 8, st, [&] {
                hipLaunchKernelGGL(k_lm_plan, dim3(1), dim3(1024), (size_t)2 * (b.nlist + 1) * 4, st, asg, (int)nqp, (int)b.nlist, h->list_off(),
                                   h->lm_qinfo.as<LmQuery>(), h->lm_items.as<LmItem>(), h->lm_n.as<int>(), (int)std::min<int64_t>(h->lm_cap_items, 0x7fffffff));
            });
            // (flops / bytes: the SURVEY 8d model -- N / nlist rows per query -- as for the query-major kernel, so that the roofline
            //  lines of the two paths compare)
            h->prof.launch("ivf_scan", 2.0 * nqp * rows * d, (double)nqp * rows * (4.0 * d + 8) + (double)nqp * d * 4, st, [&] {
                const int grid = (int)std::min<int64_t>(h->lm_cap_items, (int64_t)num_cus() * 3);
                hipLaunchKernelGGL(k_lm_gemm, dim3((unsigned)std::max(grid, 1)), dim3(256), 0, st, qp, h->lm_qinfo.as<LmQuery>(), h->vecs(), h->lm_rn.as<float>(),
                                   h->list_off(), h->lm_items.as<LmItem>(), h->lm_n.as<int>(), d, pitch, h->lm_S.as<float>());
            });
            h->prof.launch("ivf_select", 3.0 * nqp * 12 * d, (double)nqp * (12.0 * d * 4 + pitch * 4.0 + d * 8.0), st, [&] {
                auto kern = d == 768 ? &k_lm_select<3> : (d == 256 ? &k_lm_select<1> : &k_lm_select<0>);
                hipLaunchKernelGGL(kern, dim3((unsigned)((nqp + 3) / 4)), dim3(256), (size_t)4 * ((size_t)std::min(pitch, LM_MAXPITCH) * 4 + LM_WAVE_EXTRA), st, qp,
                                   h->lm_qinfo.as<LmQuery>(), h->ids(), h->vecs(), h->lm_S.as<float>(), (int)nqp, (int)b.nlist, d, pitch, h->lm_vmax, k, D + qs * k,
                                   I + qs * k, h->P.as<int64_t>() + qs * k, h->flag.as<int>(), bf ? bf->feats + qs * d : nullptr, bf ? bf->rate : 0.f,
                                   bf ? bf->omr : 0.f, h->hdr.pos_last);
            });
        }
        HIP_CHECK(hipGetLastError());
        return bf != nullptr;
    }
    // list-sorted, XCD-contiguous query order for the specialised scans (see k_qsort_hist)
    const int* perm = nullptr;
    if (np == 1 && nq >= 64 && nq < (1ll << 31) && (d == 768 || d == 256) && !h->opt.on("IVF_GENERIC") && h->opt.geti("IVF_SORT", 0)) {
        h->prof.launch("ivf_sort", 0.0, (double)nq * 16 + (double)b.nlist * 8, st, [&] {
            HIP_CHECK(hipMemsetAsync(h->qcnt.p, 0, (size_t)(b.nlist + 1) * 4, st));
            hipLaunchKernelGGL(k_qsort_hist, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, h->assign.as<int64_t>(), nq, b.nlist, h->qcnt.as<int>());
            hipLaunchKernelGGL(k_qsort_scan, dim3(1), dim3(1024), 0, st, h->qcnt.as<int>(), b.nlist + 1);
            hipLaunchKernelGGL(k_qsort_scatter, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, h->assign.as<int64_t>(), nq, b.nlist, h->qcnt.as<int>(),
                               h->qperm.as<int>());
        });
        perm = h->qperm.as<int>();
    }
    bool fused = false;
    const double rows = b.nlist ? (double)b.ntotal / (double)b.nlist * np : 0;
    const size_t smem = align_up((size_t)d * 4, 16) + SCAN_GROUPS * sizeof(TopK);
    h->prof.launch("ivf_scan", 3.0 * nq * rows * d, (double)nq * rows * (4.0 * d + 8) + (double)nq * d * 4, st, [&] {
        const size_t sm2 = SCAN_GROUPS * sizeof(TopK);
        if (d == 768 && !h->opt.on("IVF_GENERIC")) {
            static unsigned long long* tsd = nullptr;
            const bool want_ts = h->opt.on("IVF_STAMPS");
            if (want_ts && !tsd) HIP_CHECK(hipMalloc(&tsd, 16 * 8));
            if (want_ts) HIP_CHECK(hipMemsetAsync(tsd, 0, 16 * 8, st));
            hipLaunchKernelGGL((k_scan_v<6, 32, 2>), dim3((unsigned)nq), dim3(256), sm2, st, q, h->assign.as<int64_t>(), np, h->list_off(),
                               h->ids(), h->vecs(), nq, k, D, I, h->P.as<int64_t>(), h->flag.as<int>(), bf ? bf->feats : nullptr,
                               bf ? bf->rate : 0.f, bf ? bf->omr : 0.f, h->hdr.pos_last, want_ts ? tsd : nullptr, perm);
            if (want_ts) {
                HIP_CHECK(hipStreamSynchronize(st));
                unsigned long long t[16];
                HIP_CHECK(hipMemcpy(t, tsd, sizeof(t), hipMemcpyDeviceToHost));
                fprintf(stderr, "[ivf stamps] (10 ns units, block 0) assign %llu list_off %llu it0 %llu it1 %llu it2 %llu loop_end %llu barrier %llu merge+blend %llu total %llu\n",
                        t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] ? t[4] - t[3] : 0, t[5] ? t[5] - t[4] : 0, t[6] - (t[5] ? t[5] : (t[4] ? t[4] : t[3])), t[7] - t[6], t[8] - t[7], t[8] - t[0]);
            }
            fused = bf != nullptr;
            return;
        }
        if (d == 256 && !h->opt.on("IVF_GENERIC")) {
            hipLaunchKernelGGL((k_scan_v<4, 16, 2>), dim3((unsigned)nq), dim3(256), sm2, st, q, h->assign.as<int64_t>(), np, h->list_off(),
                               h->ids(), h->vecs(), nq, k, D, I, h->P.as<int64_t>(), h->flag.as<int>(), bf ? bf->feats : nullptr,
                               bf ? bf->rate : 0.f, bf ? bf->omr : 0.f, h->hdr.pos_last, nullptr, perm);
            fused = bf != nullptr;
            return;
        }
        hipLaunchKernelGGL(k_scan, dim3((unsigned)nq), dim3(256), smem, st, q, h->assign.as<int64_t>(), np,
                           h->list_off(), h->ids(), h->vecs(), nq, d, k, D, I, h->P.as<int64_t>(), h->flag.as<int>(),
                           h->opt.geti("IVF_DBG", 0));
    });
    HIP_CHECK(hipGetLastError());
    return fused;
}

// Exact (fp64-verified) nearest centroid of n device rows: the search path's own prefilter + verification kernels (ties -> lowest
// list id), in chunks of `chunk` rows -- the size `S` (chunk x nlist fp32 scores) was allocated for.  Shared by the k-means
// iterations of the build and by rvcmi_ivf_add: there is one assignment rule.
static int64_t coarse_chunk(int64_t n, int64_t nlist) {
    return std::max<int64_t>(64, std::min<int64_t>(n, ((int64_t)512 << 20) / (4 * nlist)));
}
static void coarse_assign_exact(const float* x, int64_t n, const float* cent, const float* cn, double cmax, int64_t nlist, int d, float* S,
                                int64_t chunk, int64_t* assign, hipStream_t st) {
    for (int64_t qs = 0; qs < n; qs += chunk) {
        const int64_t nqc = std::min<int64_t>(chunk, n - qs);
        const float* q = x + qs * d;
        if (((nlist + 127) / 128) * ((nqc + 63) / 64) >= 512) {
            dim3 grid((unsigned)((nlist + 127) / 128), (unsigned)((nqc + 63) / 64));
            hipLaunchKernelGGL((k_coarse_gemm<2, 4>), grid, dim3(256), 0, st, q, cent, cn, nqc, nlist, d, S);
        } else {
            dim3 grid((unsigned)((nlist + 31) / 32), (unsigned)((nqc + 31) / 32));
            hipLaunchKernelGGL((k_coarse_gemm<1, 1>), grid, dim3(64), 0, st, q, cent, cn, nqc, nlist, d, S);
        }
        hipLaunchKernelGGL(k_coarse_pick, dim3((unsigned)((nqc + 3) / 4)), dim3(256), 0, st, q, cent, S, nqc, nlist, d, cmax, assign + qs);
    }
    HIP_CHECK(hipGetLastError());
}

// index.add of n device rows (ivf_add_kernels.hpp).  assign_dev: their nearest centroids when the caller has them already (the
// build's last assignment pass), else nullptr.  Allocates, synchronises `st`, replaces h->blob.
static void ivf_add_device(rvcmi_ivf* h, int64_t n, const float* x_dev, const int64_t* assign_dev, hipStream_t st) {
    const BlobHeader ob = h->hdr;
    const int d = ob.d;
    const int64_t nlist = ob.nlist, nt0 = ob.ntotal, nt1 = nt0 + n;
    BlobHeader nh = ob;
    nh.ntotal = nt1;
    blob_layout(nh);
    DevBuf As, Sc, Cnt, Cur, NB;
    if (!assign_dev) {
        As.alloc((size_t)n * 8);
        const int64_t chunk = coarse_chunk(n, nlist);
        Sc.alloc((size_t)chunk * nlist * 4);
        coarse_assign_exact(x_dev, n, h->centroids(), h->cnorm(), ob.cmax, nlist, d, Sc.as<float>(), chunk, As.as<int64_t>(), st);
        assign_dev = As.as<int64_t>();
    }
    Cnt.alloc((size_t)(nlist + 1) * 8);
    Cur.alloc((size_t)(nlist + 1) * 8);
    NB.alloc((size_t)nh.total_bytes);
    char* nb = NB.as<char>();
    // (the whole blob, padding included, is a function of the old index and x: blob() hands these bytes out)
    HIP_CHECK(hipMemsetAsync(nb, 0, (size_t)nh.total_bytes, st));
    HIP_CHECK(hipMemsetAsync(Cnt.p, 0, (size_t)(nlist + 1) * 8, st));
    HIP_CHECK(hipMemcpyAsync(nb + nh.off_centroids, h->blob + ob.off_centroids, (size_t)nlist * d * 4, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(nb + nh.off_centroids_t, h->blob + ob.off_centroids_t, (size_t)nlist * d * 4, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(nb + nh.off_cnorm, h->blob + ob.off_cnorm, (size_t)nlist * 4, hipMemcpyDeviceToDevice, st));
    int64_t* new_off = (int64_t*)(nb + nh.off_list_offsets);
    int64_t* new_ids = (int64_t*)(nb + nh.off_ids);
    const unsigned nblk = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_add_count, dim3(nblk), dim3(256), 0, st, assign_dev, n, nlist, Cnt.as<unsigned long long>());
    hipLaunchKernelGGL(k_add_offsets, dim3(1), dim3(1024), 0, st, Cnt.as<unsigned long long>(), nlist, h->list_off(), assign_dev, n, new_off,
                       Cur.as<unsigned long long>());
    hipLaunchKernelGGL(k_add_claim, dim3(nblk), dim3(256), 0, st, assign_dev, n, nlist, nt0, Cur.as<unsigned long long>(), new_ids);
    hipLaunchKernelGGL(k_add_sort, dim3((unsigned)nlist), dim3(1024), 0, st, h->list_off(), new_off, new_ids);
    hipLaunchKernelGGL(k_add_fill, dim3((unsigned)((nt1 + 3) / 4)), dim3(256), 0, st, h->list_off(), new_off, nlist, h->ids(), h->vecs(), x_dev, nt0,
                       nt1, d, new_ids, (float*)(nb + nh.off_vecs));
    HIP_CHECK(hipGetLastError());
    unsigned long long pos_last = 0;
    HIP_CHECK(hipMemcpyAsync(&pos_last, Cur.as<unsigned long long>() + nlist, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    nh.pos_last = (int64_t)pos_last;
    HIP_CHECK(hipMemcpy(nb, &nh, sizeof(BlobHeader), hipMemcpyHostToDevice));
    // the new blob is live: an adopted old blob stays with its owner, an owned one is freed
    if (h->owns_blob && h->blob) (void)hipFree(h->blob);
    h->blob = nb;
    NB.p = nullptr;
    NB.bytes = 0;
    h->owns_blob = true;
    h->hdr = nh;
    // everything derived from the stored rows is stale (row norms, the largest norm -- the error bound of the list-major prefilter --,
    // the longest list and the item capacity sized from it): dropped here and rebuilt for the capacity the handle had reserved
    const int64_t want = h->cap_nq;
    h->lm_ready = false;
    h->lm_vmax = 0.0;
    h->lm_maxlen = h->lm_cap_items = h->lm_cap_nq = h->lm_buf_nq = 0;
    h->cap_nq = 0;
    if (want > 0) reserve(h, want);
}

static rvcmi_ivf* empty_index(int d, int64_t nlist, int nprobe, const float* centroids, int device) {
    const std::vector<int64_t> off((size_t)nlist + 1, 0);
    return from_host_blob(build_blob(d, 0, nlist, nprobe, centroids, off.data(), nullptr, nullptr), device);
}

// shared by rvcmi_ivf_build (centroids_out == nullptr: k-means + add -> *out) and rvcmi_kmeans (centroids only: niter Lloyd updates, no
// final assignment pass, no list-major copy of the vectors, no index object).  The host steps are those of ivf_kmeans.hpp.
static void ivf_build_impl(int d, int64_t n, const float* x_host, int64_t nlist, int niter, uint64_t seed, int device,
                           double* objective_out, float* centroids_out, rvcmi_ivf** out) {
    if (!x_host || (!out && !centroids_out)) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
    DeviceGuard dg(device);
    validate(d, n, nlist, 1);
    if (n < nlist) RVCMI_FAIL(RVCMI_ERR_INVALID, "need at least nlist=%lld training vectors, got %lld", (long long)nlist, (long long)n);
    if (niter < 0 || niter > 1000) RVCMI_FAIL(RVCMI_ERR_INVALID, "niter out of range");
    hipStream_t st = nullptr;
    DevBuf X, Cd, Cn, Sc, As, Ord, Off, Dist;
    X.alloc((size_t)n * d * 4);
    HIP_CHECK(hipMemcpy(X.p, x_host, (size_t)n * d * 4, hipMemcpyHostToDevice));
    Cd.alloc((size_t)nlist * d * 4);
    Cn.alloc((size_t)nlist * 4);
    As.alloc((size_t)n * 8);
    Ord.alloc((size_t)n * 8);
    Off.alloc((size_t)(nlist + 1) * 8);
    Dist.alloc((size_t)n * 8);
    const int64_t chunk = coarse_chunk(n, nlist);
    Sc.alloc((size_t)chunk * nlist * 4);
    std::vector<float> cent((size_t)nlist * d);
    {
        const std::vector<int64_t> rows = kmeans_seed_rows(n, nlist, seed);
        for (int64_t i = 0; i < nlist; ++i) memcpy(&cent[(size_t)i * d], x_host + (size_t)rows[i] * d, (size_t)d * 4);
    }
    std::vector<int64_t> assign(n), order(n), off(nlist + 1);
    std::vector<float> cn(nlist);
    std::vector<double> dist(n);
    for (int it = 0; it <= niter; ++it) {
        if (centroids_out && it == niter) break;  // centres only: the assignment after the last update is not needed
        const double cmax = centroid_norms(cent.data(), nlist, d, cn.data());
        HIP_CHECK(hipMemcpyAsync(Cd.p, cent.data(), cent.size() * 4, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(Cn.p, cn.data(), cn.size() * 4, hipMemcpyHostToDevice, st));
        // exact (fp64-verified) nearest centroid of every training vector: the search path's own coarse kernels
        coarse_assign_exact(X.as<float>(), n, Cd.as<float>(), Cn.as<float>(), cmax, nlist, d, Sc.as<float>(), chunk, As.as<int64_t>(), st);
        if (objective_out) {
            hipLaunchKernelGGL(k_assigned_dist, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, X.as<float>(), Cd.as<float>(),
                               As.as<int64_t>(), n, d, Dist.as<double>());
            HIP_CHECK(hipMemcpyAsync(dist.data(), Dist.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        }
        // (the assignment after the last update stays on the device: the add below places the rows from it)
        if (it < niter) HIP_CHECK(hipMemcpyAsync(assign.data(), As.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (objective_out) {
            double o = 0.0;
            for (int64_t i = 0; i < n; ++i) o += dist[i];
            objective_out[it] = o;
        }
        if (it == niter) break;
        kmeans_lists(assign.data(), n, nlist, off, order);
        HIP_CHECK(hipMemcpyAsync(Ord.p, order.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(Off.p, off.data(), (size_t)(nlist + 1) * 8, hipMemcpyHostToDevice, st));
        // Lloyd update: every non-empty list's centre <- the mean of its rows
        hipLaunchKernelGGL(k_list_mean, dim3((unsigned)nlist), dim3(256), 0, st, X.as<float>(), Ord.as<int64_t>(), Off.as<int64_t>(), d,
                           Cd.as<float>());
        HIP_CHECK(hipMemcpyAsync(cent.data(), Cd.p, cent.size() * 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        kmeans_split_empty(cent.data(), nlist, d, off.data());
        // relocation (kmeans_relocate), while settling iterations remain: its inputs are computed here on the device, from the device's copy of
        // the new means -- the split above touched the host copy only (an empty list still holds its previous centre in Cd), while the costs
        // inside kmeans_relocate are taken on the host centres after the split.  oracle/ivf_build_oracle.py restates exactly this.
        if (it + 3 < niter && nlist >= 2) {
            hipLaunchKernelGGL(k_assigned_dist, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, X.as<float>(), Cd.as<float>(), As.as<int64_t>(), n, d,
                               Dist.as<double>());  // distance of every row to ITS new mean
            HIP_CHECK(hipMemcpyAsync(dist.data(), Dist.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
            // nearest OTHER centre of every centre: the two nearest centres of the new means (fp64, the nprobe > 1 kernels)
            const int64_t cch = std::max<int64_t>(1, std::min<int64_t>(nlist, ((int64_t)256 << 20) / (8 * nlist)));
            DevBuf CC, NN;
            CC.alloc((size_t)cch * nlist * 8);
            NN.alloc((size_t)nlist * 2 * 8);
            for (int64_t cs = 0; cs < nlist; cs += cch) {
                const int64_t nc = std::min<int64_t>(cch, nlist - cs);
                hipLaunchKernelGGL(k_coarse_dist, dim3((unsigned)((nc * nlist + 255) / 256)), dim3(256), 0, st, Cd.as<float>() + cs * d, Cd.as<float>(), nc,
                                   nlist, d, CC.as<double>());
                hipLaunchKernelGGL(k_coarse_select, dim3((unsigned)nc), dim3(64), 0, st, CC.as<double>(), nlist, 2, NN.as<int64_t>() + cs * 2);
            }
            HIP_CHECK(hipGetLastError());
            std::vector<int64_t> nn2((size_t)nlist * 2);
            HIP_CHECK(hipMemcpyAsync(nn2.data(), NN.p, nn2.size() * 8, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            kmeans_relocate(x_host, d, nlist, dist.data(), nn2.data(), off.data(), order.data(), cent.data());
        }
    }
    // every centre is finite and usable: a cluster that lost all its points was re-seeded by splitting the largest one.  Not every centre is
    // distinct or has points: an all-zero centre cannot be split, and more lists than distinct rows leave duplicates of the seeds' rows
    if (centroids_out) {
        memcpy(centroids_out, cent.data(), cent.size() * 4);
        return;
    }
    // index.add: the trained, empty index takes every row by the device-side add (the last assignment pass above is its input)
    Sc.free();
    Ord.free();
    Off.free();
    Dist.free();
    std::unique_ptr<rvcmi_ivf> h(empty_index(d, nlist, 1, cent.data(), device));
    ivf_add_device(h.get(), n, X.as<float>(), As.as<int64_t>(), st);
    *out = h.release();
}

}  // namespace rvcmi

extern "C" {

int rvcmi_ivf_create_from_file(const char* path, int device, rvcmi_ivf** out) {
    return guarded([&] {
        if (!path || !out) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        *out = read_faiss(path, device);
    });
}
int rvcmi_ivf_write_file(const rvcmi_ivf* h, const char* path) {
    return guarded([&] {
        if (!h || !path) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        DeviceGuard dg(h->device);
        write_faiss(h, path);
    });
}
int rvcmi_ivf_build(int d, int64_t n, const float* x_host, int64_t nlist, int niter, uint64_t seed, int device,
                    double* objective_out, rvcmi_ivf** out) {
    return guarded([&] {
        if (!out) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        ivf_build_impl(d, n, x_host, nlist, niter, seed, device, objective_out, nullptr, out);
    });
}
int rvcmi_kmeans(int d, int64_t n, const float* x_host, int64_t k, int niter, uint64_t seed, int device, double* objective_out,
                 float* centroids_out_host) {
    return guarded([&] {
        if (!centroids_out_host) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        ivf_build_impl(d, n, x_host, k, niter, seed, device, objective_out, centroids_out_host, nullptr);
    });
}
int rvcmi_ivf_train(int d, int64_t n, const float* x_host, int64_t nlist, int niter, uint64_t seed, int device, double* objective_out,
                    rvcmi_ivf** out) {
    return guarded([&] {
        if (!out) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        validate(d, n, nlist, 1);
        std::vector<float> cent((size_t)nlist * d);
        ivf_build_impl(d, n, x_host, nlist, niter, seed, device, objective_out, cent.data(), nullptr);
        *out = empty_index(d, nlist, 1, cent.data(), device);
    });
}
int rvcmi_ivf_add(rvcmi_ivf* h, int64_t n, const float* x, int x_on_device, void* stream) {
    return guarded([&] {
        if (!h || h->hdr.magic != kMagic || !h->blob) RVCMI_FAIL(RVCMI_ERR_INVALID, "add: not a trained rvcmi IVF index");
        if (n < 0) RVCMI_FAIL(RVCMI_ERR_INVALID, "add: n=%lld is negative", (long long)n);
        if (n == 0) return;
        if (!x) RVCMI_FAIL(RVCMI_ERR_INVALID, "add: null x with n=%lld", (long long)n);
        const int64_t lim = (int64_t)(((uint64_t)1 << 62) / ((uint64_t)h->hdr.d * 4));  // the vectors section stays below 2^62 bytes
        if (n > lim || h->hdr.ntotal > lim - n)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "add: ntotal %lld + n %lld overflows the index", (long long)h->hdr.ntotal, (long long)n);
        DeviceGuard dg(h->device);
        hipStream_t st = (hipStream_t)stream;
        DevBuf X;
        if (!x_on_device) {
            X.alloc((size_t)n * h->hdr.d * 4);
            HIP_CHECK(hipMemcpyAsync(X.p, x, (size_t)n * h->hdr.d * 4, hipMemcpyHostToDevice, st));
            x = X.as<float>();
        }
        ivf_add_device(h, n, x, nullptr, st);
    });
}
int rvcmi_ivf_create(int d, int64_t n, int64_t nlist, int nprobe, const float* centroids, const int64_t* list_offsets,
                     const int64_t* ids, const float* vecs, int device, rvcmi_ivf** out) {
    return guarded([&] {
        if (!centroids || !list_offsets || !out || (n && (!ids || !vecs))) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        auto blob = build_blob(d, n, nlist, nprobe, centroids, list_offsets, ids, vecs);
        *out = from_host_blob(blob, device);
    });
}
int rvcmi_ivf_destroy(rvcmi_ivf* h) {
    return guarded([&] { delete h; });
}
int rvcmi_ivf_d(const rvcmi_ivf* h) { return h ? h->hdr.d : RVCMI_ERR_INVALID; }
int64_t rvcmi_ivf_ntotal(const rvcmi_ivf* h) { return h ? h->hdr.ntotal : RVCMI_ERR_INVALID; }
int64_t rvcmi_ivf_nlist(const rvcmi_ivf* h) { return h ? h->hdr.nlist : RVCMI_ERR_INVALID; }
int rvcmi_ivf_nprobe(const rvcmi_ivf* h) { return h ? h->hdr.nprobe : RVCMI_ERR_INVALID; }
int rvcmi_ivf_set_nprobe(rvcmi_ivf* h, int nprobe) {
    return guarded([&] {
        if (!h || nprobe < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "bad nprobe");
        h->hdr.nprobe = nprobe;
        DeviceGuard dg(h->device);
        HIP_CHECK(hipMemcpy(h->blob, &h->hdr, sizeof(BlobHeader), hipMemcpyHostToDevice));
    });
}
int rvcmi_ivf_reserve(rvcmi_ivf* h, int64_t max_nq) {
    return guarded([&] {
        if (!h || max_nq < 0) RVCMI_FAIL(RVCMI_ERR_INVALID, "bad argument");
        reserve(h, max_nq);
    });
}
int rvcmi_ivf_search(rvcmi_ivf* h, int64_t nq, const float* q, int k, float* D, int64_t* I, void* stream) {
    return guarded([&] { search(h, nq, q, k, D, I, (hipStream_t)stream); });
}
int rvcmi_ivf_search_blend(rvcmi_ivf* h, int64_t nq, float* feats, float index_rate, int k, int skip_if_short, void* stream) {
    return guarded([&] {
        if (!h || (nq && !feats)) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        if (nq == 0) return;
        hipStream_t st = (hipStream_t)stream;
        reserve(h, nq);
        const int d = h->hdr.d;
        // torch evaluates `npy * index_rate + (1 - index_rate) * feats` with the python scalars cast to fp32
        const float rate = index_rate, omr = (float)(1.0 - (double)index_rate);
        const BlendFuse bf = {feats, rate, omr};
        // without the realtime guard the blend of a row needs nothing but that row's own results: done by the scan block
        if (search(h, nq, feats, k, h->Dtmp.as<float>(), h->Itmp.as<int64_t>(), st, skip_if_short ? nullptr : &bf)) return;
        h->prof.launch("ivf_blend", 2.0 * nq * k * d, (double)nq * d * 4 * (2 + k), st, [&] {
            hipLaunchKernelGGL(k_blend, dim3((unsigned)nq), dim3(256), 0, st, feats, h->Dtmp.as<float>(), h->P.as<int64_t>(),
                               h->vecs(), d, k, h->hdr.pos_last, rate, omr, h->flag.as<int>(), skip_if_short);
        });
        HIP_CHECK(hipGetLastError());
    });
}
int rvcmi_ivf_search_blend_expand(rvcmi_ivf* h, int64_t nq, const float* feats, float index_rate, int k, int skip_if_short,
                                  const float* pitchf, float protect, int64_t p_len, float* out, void* stream) {
    return guarded([&] {
        if (!h || (nq && (!feats || !out))) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        if (p_len < 0 || p_len > 2 * nq) RVCMI_FAIL(RVCMI_ERR_INVALID, "p_len %lld outside [0, 2*nq]", (long long)p_len);
        if (nq == 0 || p_len == 0) return;
        hipStream_t st = (hipStream_t)stream;
        reserve(h, nq);
        search(h, nq, feats, k, h->Dtmp.as<float>(), h->Itmp.as<int64_t>(), st);
        const int d = h->hdr.d;
        const float rate = index_rate, omr = (float)(1.0 - (double)index_rate);
        h->prof.launch("ivf_blend_x2", 2.0 * nq * k * d, (double)nq * d * 4 * (1 + k) + (double)p_len * d * 4, st, [&] {
            // one session, no skipped rows: result row qi, flags[0] = the search's any_short
            hipLaunchKernelGGL(k_blend_expand_batch, dim3((unsigned)nq, 1), dim3(256), 0, st, feats, (const float*)h->Dtmp.as<float>(),
                               (const int64_t*)h->P.as<int64_t>(), h->vecs(), d, k, h->hdr.pos_last, rate, omr, (const int*)h->flag.as<int>(),
                               skip_if_short, nq, (int64_t)0, pitchf, protect, p_len, 2, out);
        });
        HIP_CHECK(hipGetLastError());
    });
}
int rvcmi_ivf_search_blend_expand_batch(rvcmi_ivf* h, int S, int64_t nq, int64_t skip_rows, const float* feats, float index_rate, int k,
                                        int skip_if_short, const float* pitchf, float protect, int64_t p_len, float* out, void* stream) {
    return guarded([&] {
        if (!h || !feats || !out) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        if (S < 1 || S > 65535) RVCMI_FAIL(RVCMI_ERR_INVALID, "S = %d outside [1, 65535]", S);
        if (nq < 1 || nq > 0x7fffffff || skip_rows < 0 || skip_rows > nq)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "nq %lld / skip_rows %lld out of range", (long long)nq, (long long)skip_rows);
        if (p_len < 0 || p_len > 2 * nq) RVCMI_FAIL(RVCMI_ERR_INVALID, "p_len %lld outside [0, 2*nq]", (long long)p_len);
        if (p_len == 0) return;
        hipStream_t st = (hipStream_t)stream;
        const int64_t m = nq - skip_rows, rows = (int64_t)S * m;
        const int d = h->hdr.d;
        DeviceGuard dg(h->device);
        if (rows > 0) {
            reserve(h, rows);
            if (rows > h->bank_cap_rows) {
                h->bank_q.alloc((size_t)rows * d * 4);
                h->bank_cap_rows = rows;
            }
            if (S > h->bank_cap_S) {
                h->bank_flags.alloc((size_t)S * 4);
                h->bank_cap_S = S;
            }
            // every session's rows [skip_rows, nq) packed -> ONE search over S * m rows -> the guard reduced per session
            hipLaunchKernelGGL(k_gather_tail_rows, dim3((unsigned)m, (unsigned)S), dim3(256), 0, st, feats, nq, skip_rows, d, h->bank_q.as<float>());
            search(h, rows, h->bank_q.as<float>(), k, h->Dtmp.as<float>(), h->Itmp.as<int64_t>(), st);
            hipLaunchKernelGGL(k_session_short, dim3((unsigned)S), dim3(256), 0, st, (const int64_t*)h->Itmp.as<int64_t>(), m * k, h->bank_flags.as<int>());
        }
        const float rate = index_rate, omr = (float)(1.0 - (double)index_rate);
        h->prof.launch("ivf_blend_x2", 2.0 * rows * k * d, (double)rows * d * 4 * (1 + k) + (double)S * p_len * d * 4, st, [&] {
            hipLaunchKernelGGL(k_blend_expand_batch, dim3((unsigned)nq, (unsigned)S), dim3(256), 0, st, feats, (const float*)h->Dtmp.as<float>(),
                               rows > 0 ? (const int64_t*)h->P.as<int64_t>() : nullptr, h->vecs(), d, k, h->hdr.pos_last, rate, omr,
                               (const int*)h->bank_flags.as<int>(), skip_if_short, nq, skip_rows, pitchf, protect, p_len, 2, out);
        });
        HIP_CHECK(hipGetLastError());
    });
}
// The batch entry with the controls per session: only the sessions with a slot are gathered (packed by slot) and searched; the guard is
// reduced per slot; the blend maps session -> slot.  Without a handle (no index): the expansion and the per-session protect mix alone.
int rvcmi_ivf_search_blend_expand_sessions(rvcmi_ivf* h, int S, int64_t nq, int d, int64_t skip_rows, const float* feats,
                                           const rvcmi_session_blend* sess_host, const rvcmi_session_blend* sess_dev, int k, int skip_if_short,
                                           const float* pitchf, int64_t p_len, float* out, void* stream) {
    return guarded([&] {
        const char* who = "search_blend_expand_sessions";
        if (!feats || !out || !sess_dev) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: null argument", who);
        if (h && (h->hdr.magic != kMagic || !h->blob)) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: not an rvcmi IVF index", who);
        if (d < 1 || (h && d != h->hdr.d)) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: d = %d, the index has %d", who, d, h ? h->hdr.d : 0);
        SessionBlendPlan plan = {0, 0, 0};
        if (const char* why = session_blend_check(sess_host, S, nq, skip_rows, p_len, h != nullptr, pitchf != nullptr, &plan))
            RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: %s", who, why);
        if (plan.rows > 0 && (k < 1 || k > 8)) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: k = %d outside [1, 8]", who, k);
        if (p_len == 0) return;
        hipStream_t st = (hipStream_t)stream;
        const int64_t m = nq - skip_rows, rows = plan.rows;
        auto expand = [&](const float* D, const int64_t* P, const float* vecs, int64_t pos_last, const int* flags) {
            hipLaunchKernelGGL(k_blend_expand_sessions, dim3((unsigned)nq, (unsigned)S), dim3(256), 0, st, feats, D, P, vecs, d, k, pos_last,
                               sess_dev, plan.active, flags, skip_if_short, nq, skip_rows, pitchf, p_len, 2, out);
        };
        if (!h) {  // no index: every session is expanded un-blended, on the caller's current device
            expand(nullptr, nullptr, nullptr, 0, nullptr);
            HIP_CHECK(hipGetLastError());
            return;
        }
        DeviceGuard dg(h->device);
        if (rows > 0) {
            reserve(h, rows);
            if (rows > h->bank_cap_rows) {
                h->bank_q.alloc((size_t)rows * d * 4);
                h->bank_cap_rows = rows;
            }
            if (plan.active > h->bank_cap_S) {
                h->bank_flags.alloc((size_t)plan.active * 4);
                h->bank_cap_S = plan.active;
            }
            hipLaunchKernelGGL(k_gather_session_rows, dim3((unsigned)m, (unsigned)S), dim3(256), 0, st, feats, nq, skip_rows, d, sess_dev, plan.active,
                               h->bank_q.as<float>());
            search(h, rows, h->bank_q.as<float>(), k, h->Dtmp.as<float>(), h->Itmp.as<int64_t>(), st);
            hipLaunchKernelGGL(k_session_short, dim3((unsigned)plan.active), dim3(256), 0, st, (const int64_t*)h->Itmp.as<int64_t>(), m * k,
                               h->bank_flags.as<int>());
        }
        h->prof.launch("ivf_blend_x2", 2.0 * rows * k * d, (double)rows * d * 4 * (1 + k) + (double)S * p_len * d * 4, st, [&] {
            expand((const float*)h->Dtmp.as<float>(), rows > 0 ? (const int64_t*)h->P.as<int64_t>() : nullptr, h->vecs(), h->hdr.pos_last,
                   (const int*)h->bank_flags.as<int>());
        });
        HIP_CHECK(hipGetLastError());
    });
}
int rvcmi_ivf_reconstruct_n(const rvcmi_ivf* h, int64_t i0, int64_t n, float* out_host) {
    return guarded([&] {
        if (!h || !out_host) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        const BlobHeader& b = h->hdr;
        if (i0 < 0 || n < 0 || i0 + n > b.ntotal) RVCMI_FAIL(RVCMI_ERR_INVALID, "range [%lld,%lld) outside ntotal %lld",
                                                                 (long long)i0, (long long)(i0 + n), (long long)b.ntotal);
        if (!n) return;
        DeviceGuard dg(h->device);
        std::vector<int64_t> ids(b.ntotal);
        std::vector<float> vecs((size_t)b.ntotal * b.d);
        HIP_CHECK(hipMemcpy(ids.data(), h->blob + b.off_ids, ids.size() * 8, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(vecs.data(), h->blob + b.off_vecs, vecs.size() * 4, hipMemcpyDeviceToHost));
        // faiss' reconstruct_n needs a direct map and raises for ids it cannot find; here rows the index does not hold (ids
        // that are not a permutation of 0..ntotal-1, e.g. after add_with_ids) are an error too, never uninitialised memory
        std::vector<char> seen((size_t)n, 0);
        for (int64_t p = 0; p < b.ntotal; ++p) {
            const int64_t id = ids[p];
            if (id >= i0 && id < i0 + n) {
                memcpy(out_host + (size_t)(id - i0) * b.d, vecs.data() + (size_t)p * b.d, (size_t)b.d * 4);
                seen[(size_t)(id - i0)] = 1;
            }
        }
        for (int64_t i = 0; i < n; ++i)
            if (!seen[(size_t)i]) RVCMI_FAIL(RVCMI_ERR_INVALID, "reconstruct_n: id %lld is not in the index (ids are not sequential)", (long long)(i0 + i));
    });
}
int rvcmi_ivf_blob(const rvcmi_ivf* h, void** dev_ptr, size_t* bytes) {
    return guarded([&] {
        if (!h || !dev_ptr || !bytes) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        *dev_ptr = h->blob;
        *bytes = h->hdr.total_bytes;
    });
}
int rvcmi_ivf_centroids(const rvcmi_ivf* h, float* out_host) {
    return guarded([&] {
        if (!h || !out_host) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        DeviceGuard dg(h->device);
        HIP_CHECK(hipMemcpy(out_host, h->centroids(), (size_t)h->hdr.nlist * h->hdr.d * sizeof(float), hipMemcpyDeviceToHost));
    });
}
int rvcmi_ivf_blob_copy(const rvcmi_ivf* h, void* dst_dev, size_t capacity, void* stream) {
    return guarded([&] {
        if (!h || !dst_dev) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        if (capacity < h->hdr.total_bytes) RVCMI_FAIL(RVCMI_ERR_INVALID, "blob_copy: destination holds %zu bytes, the index needs %zu", capacity, (size_t)h->hdr.total_bytes);
        DeviceGuard dg(h->device);
        HIP_CHECK(hipMemcpyAsync(dst_dev, h->blob, h->hdr.total_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    });
}
int rvcmi_ivf_create_from_blob(void* dev_ptr, size_t bytes, int device, int take_ownership, rvcmi_ivf** out) {
    return guarded([&] {
        if (!dev_ptr || !out || bytes < sizeof(BlobHeader)) RVCMI_FAIL(RVCMI_ERR_INVALID, "bad blob");
        DeviceGuard dg(device);
        std::unique_ptr<rvcmi_ivf> h(new rvcmi_ivf());
        h->device = device;
        HIP_CHECK(hipMemcpy(&h->hdr, dev_ptr, sizeof(BlobHeader), hipMemcpyDeviceToHost));
        if (h->hdr.magic != kMagic || h->hdr.version != 1 || h->hdr.total_bytes != bytes)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "not an rvcmi IVF blob (magic/version/size mismatch)");
        validate(h->hdr.d, h->hdr.ntotal, h->hdr.nlist, h->hdr.nprobe);
        h->blob = (char*)dev_ptr;
        h->owns_blob = take_ownership != 0;
        *out = h.release();
    });
}
int rvcmi_ivf_set_option(rvcmi_ivf* h, const char* key, double value) {
    return guarded([&] {
        if (!h || !key) RVCMI_FAIL(RVCMI_ERR_INVALID, "null argument");
        if (!h->opt.set(key, value)) RVCMI_FAIL(RVCMI_ERR_INVALID, "unknown option '%s' for this handle", key);
    });
}
int rvcmi_ivf_profile_enable(rvcmi_ivf* h, int enable) {
    return guarded([&] {
        if (!h) RVCMI_FAIL(RVCMI_ERR_INVALID, "null handle");
        h->prof.enabled = enable != 0;
    });
}
int rvcmi_ivf_profile_read(rvcmi_ivf* h, rvcmi_kernel_stat* stats, int capacity, int* n, int reset) {
    return guarded([&] {
        if (!h) RVCMI_FAIL(RVCMI_ERR_INVALID, "null handle");
        h->prof.read(stats, capacity, n, reset);
    });
}

}  // extern "C"
