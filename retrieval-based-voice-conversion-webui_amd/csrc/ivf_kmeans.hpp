// Host steps of the k-means behind the index build (web.py:544-563: index.train), as plain functions over host arrays (no HIP):
// ivf_build_impl in ivf.hip owns the device buffers, the launches and the loop, and calls one of these per step.  Every step is
// deterministic: the built index is a function of (x, nlist, niter, seed) -- the one oracle/ivf_build_oracle.py restates step by step.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace rvcmi {

// init: nlist distinct training rows (seeded partial Fisher-Yates), like faiss' random subset initialisation
inline std::vector<int64_t> kmeans_seed_rows(int64_t n, int64_t nlist, uint64_t seed) {
    std::vector<int64_t> perm(n);
    for (int64_t i = 0; i < n; ++i) perm[i] = i;
    uint64_t sd = seed * 6364136223846793005ULL + 1442695040888963407ULL;
    for (int64_t i = 0; i < nlist; ++i) {
        sd ^= sd >> 12; sd ^= sd << 25; sd ^= sd >> 27;  // xorshift64*
        const uint64_t r = (sd * 2685821657736338717ULL) % (uint64_t)(n - i);
        std::swap(perm[i], perm[i + (int64_t)r]);
    }
    perm.resize(nlist);
    return perm;
}

// lists: stable counting sort by centroid => ids ascending inside a list (what sequential index.add produces).
// off: [nlist + 1] list offsets, order: [n] row ids, list-major
inline void kmeans_lists(const int64_t* assign, int64_t n, int64_t nlist, std::vector<int64_t>& off, std::vector<int64_t>& order) {
    off.assign(nlist + 1, 0);
    order.resize(n);
    for (int64_t i = 0; i < n; ++i) off[assign[i] + 1]++;
    for (int64_t l = 0; l < nlist; ++l) off[l + 1] += off[l];
    std::vector<int64_t> cur(off.begin(), off.end() - 1);
    for (int64_t i = 0; i < n; ++i) order[cur[assign[i]]++] = i;
}

// empty lists: split the currently largest one (faiss' split_clusters idea, deterministic choice): copy its
// centroid and nudge the two copies apart by 1/1024 in alternating coordinates.  The nudge is relative: an all-zero centre cannot be
// split (v * (1 +- 1/1024) is 0), the re-seeded list stays its duplicate and stays empty -- legal for retrieval (ties go to the lower
// list), and pinned as it is by tests/ivf_build_cases.py "zero_rows".  The running sizes make the next empty list split what is largest then.
inline void kmeans_split_empty(float* cent, int64_t nlist, int d, const int64_t* off) {
    std::vector<int64_t> sz(nlist);
    for (int64_t l = 0; l < nlist; ++l) sz[l] = off[l + 1] - off[l];
    for (int64_t l = 0; l < nlist; ++l) {
        if (sz[l]) continue;
        const int64_t big = std::max_element(sz.begin(), sz.end()) - sz.begin();
        for (int e = 0; e < d; ++e) {
            const float v = cent[big * d + e];
            const float eps = 1.f / 1024.f;
            cent[l * d + e] = (e & 1) ? v * (1.f - eps) : v * (1.f + eps);
            cent[big * d + e] = (e & 1) ? v * (1.f + eps) : v * (1.f - eps);
        }
        sz[l] = sz[big] / 2;
        sz[big] -= sz[l];
    }
}

// Relocation.  Lloyd iterations from a random start never repair "two centres inside one natural cluster, none in
// another": against the reference's MiniBatchKMeans call (web.py:522-536; it re-seeds low-count centres every batch) they ended
// 1.43x above its objective on well-separated blobs.  After the update, while settling iterations remain: the centre whose
// deletion costs least -- every point of cluster j re-assigned to j's nearest other centre i costs at most n_j |c_j - c_i|^2 --
// moves to the farthest point p of the cluster with the largest distortion, if the EXACT gain of a centre at p for that
// cluster's own points, sum max(0, |x - c_o|^2 - |x - p|^2), exceeds that cost: the objective of the next assignment cannot
// go up (the build's objective stays non-increasing over every iteration that splits no empty list; kmeans_split_empty does nudge a
// centre off its mean, so an iteration that splits may raise it).  Deterministic; at most nlist / 20 moves per iteration; on rows without
// cluster structure no move passes the test and the iterations are the plain ones.
//   dist: [n] squared distance of every row to the mean of its list;  nn2: [nlist][2] the two nearest centres of every centre (itself
//   among them);  off / order: the lists (kmeans_lists);  cent: [nlist][d], moved centres are overwritten.
// Returns the moves made: (centre, the training row it now equals).
inline std::vector<std::pair<int64_t, int64_t>> kmeans_relocate(const float* x_host, int d, int64_t nlist, const double* dist, const int64_t* nn2,
                                                                const int64_t* off, const int64_t* order, float* cent) {
    std::vector<double> S(nlist, 0.0), cost(nlist, INFINITY);
    std::vector<int64_t> nn(nlist, -1);
    for (int64_t l = 0; l < nlist; ++l)
        for (int64_t p = off[l]; p < off[l + 1]; ++p) S[l] += dist[order[p]];
    for (int64_t l = 0; l < nlist; ++l) {
        const int64_t cnt = off[l + 1] - off[l];
        if (!cnt) continue;  // (an empty list was just re-seeded by kmeans_split_empty)
        int64_t o = nn2[l * 2] == l ? nn2[l * 2 + 1] : nn2[l * 2];
        if (o < 0 || o == l || off[o + 1] == off[o]) continue;
        double dn = 0.0;
        for (int e = 0; e < d; ++e) {
            const double t = (double)cent[l * d + e] - (double)cent[o * d + e];
            dn += t * t;
        }
        nn[l] = o;
        cost[l] = (double)cnt * dn;
    }
    std::vector<int64_t> by_cost(nlist), by_S(nlist);
    for (int64_t l = 0; l < nlist; ++l) by_cost[l] = by_S[l] = l;
    std::sort(by_cost.begin(), by_cost.end(), [&](int64_t a1, int64_t b1) { return cost[a1] < cost[b1] || (cost[a1] == cost[b1] && a1 < b1); });
    std::sort(by_S.begin(), by_S.end(), [&](int64_t a1, int64_t b1) { return S[a1] > S[b1] || (S[a1] == S[b1] && a1 < b1); });
    // used[]: centres that took part in a move of this iteration (the moved centre, the split cluster, the receiving centre) -- none
    // of them is deleted or split again.  moved[]: centres that are GONE from their old place: a later candidate whose nearest centre
    // was moved has a stale cost (n_j |c_j - c_nn|^2 against a centre that is no longer there) and is skipped, so every accepted
    // move still satisfies gain > cost and the objective cannot go up.
    std::vector<char> used(nlist, 0), moved(nlist, 0);
    std::vector<std::pair<int64_t, int64_t>> moves;
    const int64_t maxmoves = std::max<int64_t>(1, nlist / 20);
    int64_t si = 0;
    for (int64_t ci = 0; ci < nlist && (int64_t)moves.size() < maxmoves; ++ci) {
        const int64_t j = by_cost[ci];
        if (used[j] || nn[j] < 0 || !(cost[j] < INFINITY) || moved[nn[j]]) continue;
        // the global cursor passes only clusters that are out for EVERY later candidate (used, or too small to split); the clusters
        // excluded for this candidate alone (j itself, its receiver) are stepped over by the local cursor
        while (si < nlist && (used[by_S[si]] || off[by_S[si] + 1] - off[by_S[si]] < 2)) ++si;
        int64_t sj = si;
        while (sj < nlist && (used[by_S[sj]] || by_S[sj] == j || by_S[sj] == nn[j] || off[by_S[sj] + 1] - off[by_S[sj]] < 2)) ++sj;
        if (sj >= nlist) break;
        const int64_t o = by_S[sj];
        int64_t far = order[off[o]];
        for (int64_t p = off[o]; p < off[o + 1]; ++p)
            if (dist[order[p]] > dist[far]) far = order[p];
        const float* xp = x_host + (size_t)far * d;
        double gain = 0.0;
        for (int64_t p = off[o]; p < off[o + 1]; ++p) {
            const float* xi = x_host + (size_t)order[p] * d;
            double dp = 0.0;
            for (int e = 0; e < d; ++e) {
                const double t = (double)xi[e] - (double)xp[e];
                dp += t * t;
            }
            gain += std::max(0.0, dist[order[p]] - dp);
        }
        if (!(gain > cost[j])) break;  // the cheapest deletion no longer pays for the best split: done for this iteration
        memcpy(&cent[(size_t)j * d], xp, (size_t)d * 4);
        used[j] = used[o] = used[nn[j]] = 1;
        moved[j] = 1;
        moves.emplace_back(j, far);
    }
    return moves;
}

}  // namespace rvcmi
