// Stand-alone host program over csrc/ivf_format.hpp and csrc/ivf_kmeans.hpp (links csrc/error.cpp, nothing else; no GPU, no HIP).
// Built and driven by tests/test_cpu_ivf_format.py; the same program is what a sanitizer build runs.
//
//   roundtrip IN OUT   parse IN, build the blob, write it to OUT, parse OUT again: the two parses must agree
//   prefixes IN TMP    every proper prefix of IN (written to TMP) must be refused with RVCMI_ERR_IO and a "truncated" message
//   reject FILE        FILE must be refused with RVCMI_ERR_IO (prints the message)
//   kmeans             the host steps of k-means on n = 64, d = 8
//   steps IN OUT       one update of the build loop on the rows, assignment and previous centres of IN (layout below): kmeans_lists ->
//                      fp64 means -> kmeans_split_empty -> kmeans_relocate; OUT = the centres and the moves
//   seeds N NLIST SEED prints kmeans_seed_rows(N, NLIST, SEED), one row per line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../retrieval-based-voice-conversion-webui_amd/csrc/ivf_format.hpp"
#include "../../retrieval-based-voice-conversion-webui_amd/csrc/ivf_kmeans.hpp"

using namespace rvcmi;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

static int parse(const char* path, FaissIvfFlat* out) {
    return guarded([&] { *out = parse_faiss(path); });
}

static int roundtrip(const char* in, const char* out) {
    FaissIvfFlat a, b;
    int rc = guarded([&] {
        a = parse_faiss(in);
        write_faiss(a.blob(), out);
        b = parse_faiss(out);
    });
    if (rc != RVCMI_OK) {
        fprintf(stderr, "roundtrip: rc=%d %s\n", rc, rvcmi_last_error());
        return 1;
    }
    CHECK(a.d == b.d && a.nprobe == b.nprobe && a.nlist == b.nlist && a.ntotal == b.ntotal);
    CHECK(a.centroids == b.centroids && a.list_offsets == b.list_offsets);
    const size_t n = (size_t)a.ntotal;
    CHECK(a.ids.size() >= n && b.ids.size() >= n && !memcmp(a.ids.data(), b.ids.data(), n * 8));
    CHECK(!memcmp(a.vecs.data(), b.vecs.data(), n * a.d * 4));
    printf("roundtrip ok: d=%d nlist=%lld ntotal=%lld\n", a.d, (long long)a.nlist, (long long)a.ntotal);
    return 0;
}

static int prefixes(const char* in, const char* tmp) {
    std::vector<char> buf;
    {
        FILE* f = fopen(in, "rb");
        CHECK(f);
        char chunk[4096];
        size_t got;
        while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
        fclose(f);
    }
    FaissIvfFlat x;
    CHECK(parse(in, &x) == RVCMI_OK);
    for (size_t len = 0; len < buf.size(); ++len) {
        FILE* f = fopen(tmp, "wb");
        CHECK(f);
        CHECK(fwrite(buf.data(), 1, len, f) == len);
        fclose(f);
        const int rc = parse(tmp, &x);
        if (rc != RVCMI_ERR_IO || !strstr(rvcmi_last_error(), "truncated")) {
            fprintf(stderr, "prefix of %zu bytes: rc=%d msg=%s\n", len, rc, rc ? rvcmi_last_error() : "(accepted)");
            return 1;
        }
    }
    printf("prefixes ok: %zu refused\n", buf.size());
    return 0;
}

static int reject(const char* path) {
    FaissIvfFlat x;
    const int rc = parse(path, &x);
    printf("rc=%d msg=%s\n", rc, rc ? rvcmi_last_error() : "(accepted)");
    return rc == RVCMI_ERR_IO ? 0 : 1;
}

// ---- k-means steps: n = 64 rows, d = 8, four blobs of 16 rows along coordinate 0, everything else by plain loops ----
static const int64_t N = 64;
static const int D = 8;

static std::vector<float> blobs(const float base[4]) {
    std::vector<float> x(N * D);
    for (int64_t i = 0; i < N; ++i)
        for (int e = 0; e < D; ++e) x[i * D + e] = (e == 0 ? base[i / 16] : 0.f) + 0.01f * (float)((i * 7 + e * 3) % 5 - 2);
    return x;
}
static double dist2(const float* a, const float* b) {
    double s = 0.0;
    for (int e = 0; e < D; ++e) s += ((double)a[e] - (double)b[e]) * ((double)a[e] - (double)b[e]);
    return s;
}
static std::vector<float> means(const std::vector<float>& x, const std::vector<int64_t>& assign, int64_t nlist) {
    std::vector<double> acc(nlist * D, 0.0);
    std::vector<int64_t> cnt(nlist, 0);
    for (int64_t i = 0; i < N; ++i) {
        cnt[assign[i]]++;
        for (int e = 0; e < D; ++e) acc[assign[i] * D + e] += x[i * D + e];
    }
    std::vector<float> c(nlist * D, 0.f);
    for (int64_t l = 0; l < nlist; ++l)
        for (int e = 0; e < D; ++e) c[l * D + e] = cnt[l] ? (float)(acc[l * D + e] / (double)cnt[l]) : 0.f;
    return c;
}
static int64_t nearest(const float* p, const std::vector<float>& cent, int64_t nlist, int64_t skip = -1) {
    int64_t best = -1;
    for (int64_t l = 0; l < nlist; ++l)
        if (l != skip && (best < 0 || dist2(p, &cent[l * D]) < dist2(p, &cent[best * D]))) best = l;
    return best;
}
// the inputs the build computes on the device, then kmeans_relocate
static std::vector<std::pair<int64_t, int64_t>> relocate(const std::vector<float>& x, const std::vector<int64_t>& assign, int64_t nlist,
                                                         std::vector<float>& cent) {
    std::vector<int64_t> off, order, nn2(nlist * 2);
    kmeans_lists(assign.data(), N, nlist, off, order);
    cent = means(x, assign, nlist);
    std::vector<double> dist(N);
    for (int64_t i = 0; i < N; ++i) dist[i] = dist2(&x[i * D], &cent[assign[i] * D]);
    for (int64_t l = 0; l < nlist; ++l) {
        nn2[l * 2] = nearest(&cent[l * D], cent, nlist);
        nn2[l * 2 + 1] = nearest(&cent[l * D], cent, nlist, nn2[l * 2]);
    }
    return kmeans_relocate(x.data(), D, nlist, dist.data(), nn2.data(), off.data(), order.data(), cent.data());
}

static int kmeans() {
    const int64_t nlist = 4;
    // seeds: nlist distinct rows, equal for equal seeds
    for (int64_t k : {4, 17, 64}) {
        const std::vector<int64_t> r = kmeans_seed_rows(N, k, 1234);
        CHECK((int64_t)r.size() == k && std::set<int64_t>(r.begin(), r.end()).size() == (size_t)k);
        for (int64_t v : r) CHECK(v >= 0 && v < N);
        CHECK(r == kmeans_seed_rows(N, k, 1234));
    }
    // counting sort: the offsets cover [0, n), ids ascend inside each list, every row sits in the list it is assigned to
    {
        std::vector<int64_t> assign(N), off, order;
        for (int64_t i = 0; i < N; ++i) assign[i] = (i * 5 + i / 7) % 7 == 3 ? 6 : (i * 5 + i / 7) % 7;  // 7 lists, list 3 empty
        kmeans_lists(assign.data(), N, 7, off, order);
        CHECK(off.size() == 8 && off[0] == 0 && off[7] == N && off[3] == off[4] && (int64_t)order.size() == N);
        std::set<int64_t> seen;
        for (int64_t l = 0; l < 7; ++l) {
            CHECK(off[l + 1] >= off[l]);
            for (int64_t p = off[l]; p < off[l + 1]; ++p) {
                CHECK(assign[order[p]] == l && (p == off[l] || order[p] > order[p - 1]));
                seen.insert(order[p]);
            }
        }
        CHECK((int64_t)seen.size() == N);
    }
    // split: list 3 forced empty (its blob sits in list 2); afterwards the two copies differ and every list gets rows
    {
        const float base[4] = {0.f, 10.f, 20.f, 30.f};
        const std::vector<float> x = blobs(base);
        std::vector<int64_t> assign(N), off, order;
        for (int64_t i = 0; i < N; ++i) assign[i] = std::min<int64_t>(i / 16, 2);
        kmeans_lists(assign.data(), N, nlist, off, order);
        CHECK(off[4] - off[3] == 0);
        std::vector<float> cent = means(x, assign, nlist);
        kmeans_split_empty(cent.data(), nlist, D, off.data());
        CHECK(memcmp(&cent[2 * D], &cent[3 * D], D * 4) != 0);
        std::vector<int64_t> cnt(nlist, 0);
        for (int64_t i = 0; i < N; ++i) cnt[nearest(&x[i * D], cent, nlist)]++;
        for (int64_t l = 0; l < nlist; ++l) CHECK(cnt[l] > 0);
    }
    // relocation, a move that pays: lists 0 and 1 share one natural cluster (deleting either costs 16 * 0.1^2), list 2 spans the blob
    // at 10 and half of the one at 30 (its rows at 30 gain ~178 each from a centre there)
    {
        const float base[4] = {0.f, 0.1f, 10.f, 30.f};
        std::vector<float> x = blobs(base);
        std::vector<int64_t> assign(N);
        for (int64_t i = 0; i < N; ++i) assign[i] = i < 56 ? std::min<int64_t>(i / 16, 2) : 3;
        for (int64_t i = 56; i < N; ++i) x[i * D] += 30.f;  // list 3: eight rows of its own at 60
        std::vector<float> cent;
        const auto moves = relocate(x, assign, nlist, cent);
        CHECK(moves.size() == 1 && (int64_t)moves.size() <= std::max<int64_t>(1, nlist / 20));
        const int64_t j = moves[0].first, row = moves[0].second;
        CHECK(j == 0 && row >= 48 && row < 56);  // the cheapest deletion (ties: the lower id) moves to a row of list 2 at 30
        CHECK(!memcmp(&cent[j * D], &x[row * D], D * 4));
        const std::vector<float> before = means(x, assign, nlist);
        for (int64_t l = 1; l < nlist; ++l) CHECK(!memcmp(&cent[l * D], &before[l * D], D * 4));
    }
    // relocation, no move pays: four separate blobs with a centre each (a deletion costs 16 * 10^2, a split gains a few 1e-3)
    {
        const float base[4] = {0.f, 10.f, 20.f, 30.f};
        const std::vector<float> x = blobs(base);
        std::vector<int64_t> assign(N);
        for (int64_t i = 0; i < N; ++i) assign[i] = i / 16;
        std::vector<float> cent;
        CHECK(relocate(x, assign, nlist, cent).empty());
        CHECK(cent == means(x, assign, nlist));
    }
    printf("kmeans ok\n");
    return 0;
}

// ---- one update of the build loop, as ivf_build_impl strings the host steps together, on inputs a test wrote ----
// IN:  int64 n, d, nlist; float x[n][d]; int64 assign[n]; float prev[nlist][d] (the centres before the update: an empty list keeps its own)
// OUT: float cent[nlist][d]; int64 nmoves; int64 (centre, row)[nmoves]
// The distances of the rows and the two nearest centres are computed here on the host by plain loops, from the means BEFORE the split (what
// the build's device copy holds at that point); kmeans_relocate then works on the centres after the split.
static int steps(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    CHECK(f);
    int64_t hdr[3];
    CHECK(fread(hdr, 8, 3, f) == 3);
    const int64_t n = hdr[0], nlist = hdr[2];
    const int d = (int)hdr[1];
    CHECK(n >= 1 && n <= (1 << 20) && d >= 1 && d <= 4096 && nlist >= 1 && nlist <= n);
    std::vector<float> x((size_t)n * d), cent((size_t)nlist * d);
    std::vector<int64_t> assign(n);
    CHECK(fread(x.data(), 4, x.size(), f) == x.size());
    CHECK(fread(assign.data(), 8, assign.size(), f) == assign.size());
    CHECK(fread(cent.data(), 4, cent.size(), f) == cent.size());
    fclose(f);
    for (int64_t i = 0; i < n; ++i) CHECK(assign[i] >= 0 && assign[i] < nlist);
    std::vector<int64_t> off, order;
    kmeans_lists(assign.data(), n, nlist, off, order);
    for (int64_t l = 0; l < nlist; ++l) {  // the Lloyd update of k_list_mean: ascending ids, fp64, one division
        if (off[l + 1] == off[l]) continue;
        for (int e = 0; e < d; ++e) {
            double acc = 0.0;
            for (int64_t p = off[l]; p < off[l + 1]; ++p) acc += (double)x[(size_t)order[p] * d + e];
            cent[(size_t)l * d + e] = (float)(acc / (double)(off[l + 1] - off[l]));
        }
    }
    auto d2 = [&](const float* a, const float* b) {
        double s = 0.0;
        for (int e = 0; e < d; ++e) s += ((double)a[e] - (double)b[e]) * ((double)a[e] - (double)b[e]);
        return s;
    };
    std::vector<double> dist(n);
    for (int64_t i = 0; i < n; ++i) dist[i] = d2(&x[(size_t)i * d], &cent[(size_t)assign[i] * d]);
    std::vector<int64_t> nn2((size_t)nlist * 2, -1);
    for (int64_t l = 0; l < nlist; ++l)
        for (int s = 0; s < 2 && s < nlist; ++s) {
            int64_t best = -1;
            for (int64_t c = 0; c < nlist; ++c)
                if (!(s == 1 && c == nn2[l * 2]) && (best < 0 || d2(&cent[(size_t)l * d], &cent[(size_t)c * d]) < d2(&cent[(size_t)l * d], &cent[(size_t)best * d])))
                    best = c;
            nn2[l * 2 + s] = best;
        }
    kmeans_split_empty(cent.data(), nlist, d, off.data());
    std::vector<std::pair<int64_t, int64_t>> moves;
    if (nlist >= 2) moves = kmeans_relocate(x.data(), d, nlist, dist.data(), nn2.data(), off.data(), order.data(), cent.data());
    f = fopen(out, "wb");
    CHECK(f);
    CHECK(fwrite(cent.data(), 4, cent.size(), f) == cent.size());
    const int64_t nm = (int64_t)moves.size();
    CHECK(fwrite(&nm, 8, 1, f) == 1);
    for (const auto& m : moves) {
        const int64_t pr[2] = {m.first, m.second};
        CHECK(fwrite(pr, 8, 2, f) == 2);
    }
    CHECK(fclose(f) == 0);
    printf("steps ok: n=%lld d=%d nlist=%lld moves=%lld\n", (long long)n, d, (long long)nlist, (long long)nm);
    return 0;
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "roundtrip" && argc == 4) return roundtrip(argv[2], argv[3]);
    if (cmd == "prefixes" && argc == 4) return prefixes(argv[2], argv[3]);
    if (cmd == "reject" && argc == 3) return reject(argv[2]);
    if (cmd == "kmeans" && argc == 2) return kmeans();
    if (cmd == "steps" && argc == 4) return steps(argv[2], argv[3]);
    if (cmd == "seeds" && argc == 5) {
        for (int64_t r : kmeans_seed_rows(atoll(argv[2]), atoll(argv[3]), strtoull(argv[4], nullptr, 10))) printf("%lld\n", (long long)r);
        return 0;
    }
    fprintf(stderr, "usage: %s roundtrip IN OUT | prefixes IN TMP | reject FILE | kmeans | steps IN OUT | seeds N NLIST SEED\n", argv[0]);
    return 2;
}
