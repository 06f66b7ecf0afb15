// The two data formats of the IVF index, host-only (no HIP): the device blob (header + offset-addressed sections, built on the host
// from arrays) and faiss' on-disk IndexIVFFlat ("IwFl": file -> host arrays -> blob, blob -> file).  ivf.hip copies blobs to and from
// the device; everything that knows a layout is here, so it compiles with a plain C++ compiler and runs under host sanitizers
// (tests/host/ivf_format_main.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "error.hpp"

#ifdef __HIPCC__
#define RVCMI_HD __host__ __device__
#else
#define RVCMI_HD
#endif

namespace rvcmi {

struct BlobHeader {  // first 128 bytes of the device blob; everything the kernels need is offset-addressed
    uint64_t magic;  // "RVCMIIVF"
    uint32_t version;
    int32_t d;
    int32_t nprobe;
    int32_t pad0;
    int64_t ntotal;
    int64_t nlist;
    int64_t pos_last;  // list-major position of the row whose id == ntotal-1 (numpy's big_npy[-1])
    uint64_t off_centroids, off_list_offsets, off_ids, off_vecs;
    uint64_t total_bytes;
    uint64_t off_centroids_t;  // [d/4][nlist] float4: the coarse pass reads it lane-per-centroid, coalesced
    uint64_t off_cnorm;        // [nlist] fp32(|c|^2) (rounded from fp64) for the fp32 prefilter
    double cmax;               // max |c| over the centroids (error bound of the prefilter)
    uint64_t reserved[2];
};
static_assert(sizeof(BlobHeader) == 128, "blob header must be 128 bytes");
static const uint64_t kMagic = 0x465649494d435652ull;  // "RVCMIIVF" little-endian

RVCMI_HD static inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

inline void validate(int d, int64_t n, int64_t nlist, int nprobe) {
    if (d < 4 || (d & 3)) RVCMI_FAIL(RVCMI_ERR_INVALID, "dimension %d must be a positive multiple of 4", d);
    if (n < 0 || nlist < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "bad sizes n=%lld nlist=%lld", (long long)n, (long long)nlist);
    if (nprobe < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "nprobe must be >= 1");
}

// the section offsets and the size of a blob of h.ntotal rows (h.d, h.nlist set): a function of the three sizes alone
inline void blob_layout(BlobHeader& h) {
    const uint64_t n1 = (uint64_t)std::max<int64_t>(h.ntotal, 1), nlist = (uint64_t)h.nlist, d = (uint64_t)h.d;
    uint64_t off = sizeof(BlobHeader);
    h.off_centroids = off;
    off = align_up(off + nlist * d * 4, 256);
    h.off_list_offsets = off;
    off = align_up(off + (nlist + 1) * 8, 256);
    h.off_ids = off;
    off = align_up(off + n1 * 8, 256);
    h.off_vecs = off;
    off = align_up(off + n1 * d * 4, 256);
    h.off_centroids_t = off;
    off = align_up(off + nlist * d * 4, 256);
    h.off_cnorm = off;
    off = align_up(off + nlist * 4, 256);
    h.total_bytes = off;
}

// cn[c] = fp32(|c|^2), accumulated in fp64; returns max |c|: the inputs of the fp32 coarse prefilter (k_coarse_pick's error bound)
inline double centroid_norms(const float* centroids, int64_t nlist, int d, float* cn) {
    double cmax2 = 0.0;
    for (int64_t c = 0; c < nlist; ++c) {
        double n2 = 0.0;
        for (int e = 0; e < d; ++e) n2 += (double)centroids[c * d + e] * (double)centroids[c * d + e];
        cn[c] = (float)n2;
        cmax2 = std::max(cmax2, n2);
    }
    return std::sqrt(cmax2);
}

inline std::vector<char> build_blob(int d, int64_t n, int64_t nlist, int nprobe, const float* centroids, const int64_t* list_offsets,
                                    const int64_t* ids, const float* vecs) {
    validate(d, n, nlist, nprobe);
    if (list_offsets[0] != 0 || list_offsets[nlist] != n) RVCMI_FAIL(RVCMI_ERR_INVALID, "list_offsets do not cover [0, n)");
    for (int64_t l = 0; l < nlist; ++l)
        if (list_offsets[l + 1] < list_offsets[l]) RVCMI_FAIL(RVCMI_ERR_INVALID, "list_offsets not monotone at %lld", (long long)l);
    BlobHeader h;
    memset(&h, 0, sizeof(h));
    h.magic = kMagic;
    h.version = 1;
    h.d = d;
    h.nprobe = nprobe;
    h.ntotal = n;
    h.nlist = nlist;
    h.pos_last = -1;
    for (int64_t i = 0; i < n; ++i)
        if (ids[i] == n - 1) h.pos_last = i;
    if (h.pos_last < 0) h.pos_last = n > 0 ? n - 1 : 0;
    blob_layout(h);
    std::vector<char> blob(h.total_bytes, 0);
    h.cmax = centroid_norms(centroids, nlist, d, (float*)(blob.data() + h.off_cnorm));
    memcpy(blob.data(), &h, sizeof(h));
    memcpy(blob.data() + h.off_centroids, centroids, (size_t)nlist * d * 4);
    memcpy(blob.data() + h.off_list_offsets, list_offsets, (size_t)(nlist + 1) * 8);
    {
        float* ct = (float*)(blob.data() + h.off_centroids_t);
        const int d4 = d / 4;
        for (int64_t c = 0; c < nlist; ++c)
            for (int e = 0; e < d4; ++e) memcpy(ct + ((size_t)e * nlist + c) * 4, centroids + c * d + e * 4, 16);
    }
    if (n) {
        memcpy(blob.data() + h.off_ids, ids, (size_t)n * 8);
        memcpy(blob.data() + h.off_vecs, vecs, (size_t)n * d * 4);
    }
    return blob;
}

// ---- faiss on-disk format (impl/index_write.cpp / index_read.cpp of faiss, as recalled; see
//      oracle/ivf_oracle.py for the independent python twin used to cross-check this reader) ----
struct FileCloser {
    FILE* f;
    ~FileCloser() {
        if (f) fclose(f);
    }
};

// Sequential reads that know how much of the file is left: every count the file states is held against `left` (the product with
// the element size overflow-checked) BEFORE anything is allocated or read by it.
struct Reader {
    FILE* f;
    const char* path;
    uint64_t left;  // bytes between the read position and the end of the file
    uint64_t need(uint64_t count, uint64_t each) {
        uint64_t bytes;
        if (__builtin_mul_overflow(count, each, &bytes) || bytes > left) RVCMI_FAIL(RVCMI_ERR_IO, "%s: truncated file", path);
        return bytes;
    }
    void read(void* dst, uint64_t count, uint64_t each = 1) {
        const uint64_t n = need(count, each);
        if (n && fread(dst, 1, n, f) != n) RVCMI_FAIL(RVCMI_ERR_IO, "%s: truncated file", path);
        left -= n;
    }
    void skip(uint64_t count, uint64_t each) {
        const uint64_t n = need(count, each);
        if (fseek(f, (long)n, SEEK_CUR)) RVCMI_FAIL(RVCMI_ERR_IO, "%s: truncated direct map", path);
        left -= n;
    }
    template <typename T>
    T get() {
        T v;
        read(&v, sizeof(T));
        return v;
    }
    void fourcc(char out[5]) {
        read(out, 4);
        out[4] = 0;
    }
};

inline void read_index_header(Reader& r, int& d, int64_t& ntotal, int& metric) {
    d = r.get<int32_t>();
    ntotal = r.get<int64_t>();
    (void)r.get<int64_t>();
    (void)r.get<int64_t>();
    (void)r.get<uint8_t>();  // is_trained
    metric = r.get<int32_t>();
    if (metric > 1) (void)r.get<float>();
}

struct FaissIvfFlat {  // an IndexIVFFlat file as host arrays: the arguments of build_blob
    int d = 0, nprobe = 1;
    int64_t nlist = 0, ntotal = 0;
    std::vector<float> centroids;      // [nlist][d]
    std::vector<int64_t> list_offsets;  // [nlist + 1]
    std::vector<int64_t> ids;           // [max(ntotal, 1)], list-major
    std::vector<float> vecs;            // [max(ntotal, 1)][d], list-major
    std::vector<char> blob() const {
        return build_blob(d, ntotal, nlist, nprobe, centroids.data(), list_offsets.data(), ids.data(), vecs.data());
    }
};

inline FaissIvfFlat parse_faiss(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) RVCMI_FAIL(RVCMI_ERR_IO, "cannot open '%s'", path);
    FileCloser fc{f};
    long file_size = -1;
    if (fseek(f, 0, SEEK_END) || (file_size = ftell(f)) < 0 || fseek(f, 0, SEEK_SET)) RVCMI_FAIL(RVCMI_ERR_IO, "%s: cannot take the file's size", path);
    Reader r{f, path, (uint64_t)file_size};
    FaissIvfFlat x;
    char cc[5];
    r.fourcc(cc);
    if (strcmp(cc, "IwFl")) RVCMI_FAIL(RVCMI_ERR_IO, "%s: fourcc '%s' is not an IndexIVFFlat (IwFl)", path, cc);
    int metric;
    read_index_header(r, x.d, x.ntotal, metric);
    if (metric != 1) RVCMI_FAIL(RVCMI_ERR_IO, "%s: metric %d; only METRIC_L2 (web.py:547) is supported", path, metric);
    if (x.d < 1 || x.ntotal < 0) RVCMI_FAIL(RVCMI_ERR_IO, "%s: header states d=%d ntotal=%lld", path, x.d, (long long)x.ntotal);
    const int d = x.d;
    const uint64_t nlist = r.get<uint64_t>();
    const uint64_t nprobe = r.get<uint64_t>();
    r.fourcc(cc);
    if (strcmp(cc, "IxF2") && strcmp(cc, "IxFl")) RVCMI_FAIL(RVCMI_ERR_IO, "%s: quantizer '%s' is not a flat L2 index", path, cc);
    int qd, qmetric;
    int64_t qn;
    read_index_header(r, qd, qn, qmetric);
    if (qmetric != 1) RVCMI_FAIL(RVCMI_ERR_IO, "%s: the coarse quantizer '%s' uses metric %d; only a flat L2 quantizer is supported", path, cc, qmetric);
    const uint64_t nfl = r.get<uint64_t>();
    uint64_t nld;
    if (qd != d || (uint64_t)qn != nlist || __builtin_mul_overflow(nlist, (uint64_t)d, &nld) || nfl != nld)
        RVCMI_FAIL(RVCMI_ERR_IO, "%s: quantizer shape mismatch", path);
    r.need(nfl, 4);  // (from here on nlist is bounded by the file's size)
    x.centroids.resize(nfl);
    r.read(x.centroids.data(), nfl, 4);
    const int dm_type = r.get<int8_t>();  // DirectMap::Type: 0 NoMap, 1 Array (a vector<idx_t> follows), 2 Hashtable
    if (dm_type != 0 && dm_type != 1)
        RVCMI_FAIL(RVCMI_ERR_IO, "%s: direct map type %d (Hashtable) is not supported; re-write the index without a direct map "
                   "(RVC never builds one, web.py:547-571)", path, dm_type);
    r.skip(r.get<uint64_t>(), 8);
    r.fourcc(cc);
    if (strcmp(cc, "ilar")) RVCMI_FAIL(RVCMI_ERR_IO, "%s: inverted lists '%s' are not ArrayInvertedLists", path, cc);
    const uint64_t nl2 = r.get<uint64_t>(), code_size = r.get<uint64_t>();
    if (nl2 != nlist || code_size != 4ull * d) RVCMI_FAIL(RVCMI_ERR_IO, "%s: inverted-list header mismatch", path);
    r.fourcc(cc);
    const uint64_t cnt = r.get<uint64_t>();
    std::vector<uint64_t> sizes(nlist, 0);
    if (!strcmp(cc, "full")) {
        if (cnt != nlist) RVCMI_FAIL(RVCMI_ERR_IO, "%s: 'full' size vector length", path);
        r.read(sizes.data(), cnt, 8);
    } else if (!strcmp(cc, "sprs")) {
        if (cnt & 1) RVCMI_FAIL(RVCMI_ERR_IO, "%s: 'sprs' size vector holds %llu words, not (list, size) pairs", path, (unsigned long long)cnt);
        r.need(cnt, 8);
        std::vector<uint64_t> pairs(cnt);
        r.read(pairs.data(), cnt, 8);
        for (uint64_t i = 0; i + 1 < cnt; i += 2) {
            if (pairs[i] >= nlist) RVCMI_FAIL(RVCMI_ERR_IO, "%s: sparse list id out of range", path);
            sizes[pairs[i]] = pairs[i + 1];
        }
    } else {
        RVCMI_FAIL(RVCMI_ERR_IO, "%s: unknown list size encoding '%s'", path, cc);
    }
    std::vector<int64_t>& off = x.list_offsets;
    off.assign(nlist + 1, 0);
    for (uint64_t l = 0; l < nlist; ++l)
        if (sizes[l] > (uint64_t)INT64_MAX || __builtin_add_overflow(off[l], (int64_t)sizes[l], &off[l + 1]))
            RVCMI_FAIL(RVCMI_ERR_IO, "%s: the list sizes overflow (list %llu holds %llu rows)", path, (unsigned long long)l, (unsigned long long)sizes[l]);
    const int64_t n = off[nlist];
    if (n != x.ntotal) RVCMI_FAIL(RVCMI_ERR_IO, "%s: lists hold %lld rows, header says %lld", path, (long long)n, (long long)x.ntotal);
    r.need((uint64_t)n, 4ull * d + 8);  // every list's size * (4 d + 8) bytes, all lists together
    x.vecs.resize((size_t)std::max<int64_t>(n, 1) * d);
    x.ids.resize(std::max<int64_t>(n, 1));
    for (uint64_t l = 0; l < nlist; ++l) {
        if (!sizes[l]) continue;
        r.read(x.vecs.data() + (size_t)off[l] * d, sizes[l] * d, 4);
        r.read(x.ids.data() + off[l], sizes[l], 8);
    }
    x.nlist = (int64_t)nlist;
    x.nprobe = (int)std::max<uint64_t>(1, nprobe);
    return x;
}

// host blob -> IndexIVFFlat file
inline void write_faiss(const std::vector<char>& blob, const char* path) {
    BlobHeader b;
    memcpy(&b, blob.data(), sizeof(b));
    FILE* f = fopen(path, "wb");
    if (!f) RVCMI_FAIL(RVCMI_ERR_IO, "cannot create '%s'", path);
    FileCloser fc{f};
    auto put = [&](const void* p, size_t n) {
        if (n && fwrite(p, 1, n, f) != n) RVCMI_FAIL(RVCMI_ERR_IO, "%s: short write", path);
    };
    auto header = [&](int32_t d, int64_t nt) {
        int64_t dummy = 1 << 20;
        uint8_t trained = 1;
        int32_t metric = 1;
        put(&d, 4); put(&nt, 8); put(&dummy, 8); put(&dummy, 8); put(&trained, 1); put(&metric, 4);
    };
    const uint64_t nlist = b.nlist, nprobe = b.nprobe;
    put("IwFl", 4);
    header(b.d, b.ntotal);
    put(&nlist, 8); put(&nprobe, 8);
    put("IxF2", 4);
    header(b.d, b.nlist);
    const uint64_t nfl = nlist * (uint64_t)b.d;
    put(&nfl, 8);
    put(blob.data() + b.off_centroids, nfl * 4);
    int8_t dm = 0;
    uint64_t zero = 0;
    put(&dm, 1); put(&zero, 8);
    put("ilar", 4);
    const uint64_t code_size = 4ull * b.d;
    put(&nlist, 8); put(&code_size, 8);
    const int64_t* off = (const int64_t*)(blob.data() + b.off_list_offsets);
    uint64_t nonzero = 0;
    for (uint64_t l = 0; l < nlist; ++l) nonzero += off[l + 1] > off[l];
    if (nonzero > nlist / 2) {
        put("full", 4);
        put(&nlist, 8);
        for (uint64_t l = 0; l < nlist; ++l) { uint64_t s = off[l + 1] - off[l]; put(&s, 8); }
    } else {
        put("sprs", 4);
        uint64_t cnt = nonzero * 2;
        put(&cnt, 8);
        for (uint64_t l = 0; l < nlist; ++l)
            if (off[l + 1] > off[l]) { uint64_t s = off[l + 1] - off[l]; put(&l, 8); put(&s, 8); }
    }
    for (uint64_t l = 0; l < nlist; ++l) {
        const uint64_t s = off[l + 1] - off[l];
        if (!s) continue;
        put(blob.data() + b.off_vecs + (size_t)off[l] * b.d * 4, s * b.d * 4);
        put(blob.data() + b.off_ids + (size_t)off[l] * 8, s * 8);
    }
}

}  // namespace rvcmi
