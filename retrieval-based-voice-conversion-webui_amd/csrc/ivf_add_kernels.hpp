// index.add on the device (web.py:561-563: `index.add(big_npy[i : i + batch_size_add])`): the rows of a batch are appended to the
// inverted lists of their nearest centroids, ids ntotal .. ntotal + n - 1, without a host hop.  Included by ivf.hip (after the coarse
// kernels of ivf_kernels.hpp, whose exact assignment is the input here).
//
// The new blob has the layout of build_blob for ntotal + n rows.  With cnt[l] = new rows of list l and shift = exclusive scan of cnt:
//   new_off[l]            = old_off[l] + shift[l]
//   old rows of list l    : old position p  ->  p + shift[l]
//   new rows of list l    : [old_off[l + 1] + shift[l], new_off[l + 1]), in ascending id order
// Determinism: the counts are integer sums (order-free); the slot a new row claims inside its segment depends on the order the
// atomics arrive in, but every id of a segment is unique and the segment is sorted by id before any row is placed, so the final
// ids array -- and with it the rows, which are gathered BY id -- is a function of (old index, assignment) alone.  No float atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rvcmi {

// a row without a nearest centroid (NaN coordinates: k_coarse_pick finds no candidate) goes to list 0, never out of bounds
__device__ __forceinline__ int64_t add_list_of(int64_t l, int64_t nlist) { return (l < 0 || l >= nlist) ? 0 : l; }

__global__ void __launch_bounds__(256) k_add_count(const int64_t* __restrict__ assign, int64_t n, int64_t nlist,
                                                   unsigned long long* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(&cnt[add_list_of(assign[i], nlist)], 1ull);
}

// One block.  cnt [nlist + 1] (counts, last entry 0) -> exclusive scan in place (cnt[nlist] = n); new_off [nlist + 1];
// cursor[l] = first slot of list l's new segment; cursor[nlist] = list-major position of id ntotal + n - 1 (the header's pos_last:
// the largest id is the last row of its list).
__global__ void __launch_bounds__(1024) k_add_offsets(unsigned long long* __restrict__ cnt, int64_t nlist, const int64_t* __restrict__ old_off,
                                                      const int64_t* __restrict__ assign, int64_t n, int64_t* __restrict__ new_off,
                                                      unsigned long long* __restrict__ cursor) {
    __shared__ unsigned long long part[1024];
    const int64_t m = nlist + 1;
    const int64_t per = (m + 1023) / 1024;
    const int64_t b = min((int64_t)threadIdx.x * per, m), e = min(b + per, m);
    unsigned long long s = 0;
    for (int64_t i = b; i < e; ++i) s += cnt[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const unsigned long long v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long run = part[threadIdx.x] - s;
    for (int64_t i = b; i < e; ++i) {
        const unsigned long long c = cnt[i];
        cnt[i] = run;
        new_off[i] = old_off[i] + (int64_t)run;
        if (i < nlist) cursor[i] = (unsigned long long)old_off[i + 1] + run;
        run += c;
    }
    __syncthreads();  // (block-wide visibility of the scanned counts)
    if (threadIdx.x == 0) {
        const int64_t l = add_list_of(assign[n - 1], nlist);
        cursor[nlist] = (unsigned long long)old_off[l + 1] + cnt[l + 1] - 1ull;
    }
}

// every new row claims a slot of its list's new segment (any order) and leaves its id there
__global__ void __launch_bounds__(256) k_add_claim(const int64_t* __restrict__ assign, int64_t n, int64_t nlist, int64_t ntotal,
                                                   unsigned long long* __restrict__ cursor, int64_t* __restrict__ new_ids) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) new_ids[atomicAdd(&cursor[add_list_of(assign[i], nlist)], 1ull)] = ntotal + i;
}

// Ascending bitonic network over a[0, m), m arbitrary: every compare-exchange leaves the smaller value at the lower index (each
// merge starts with the mirrored step i <-> i ^ (k - 1) instead of alternating directions), so the virtual +inf padding up to the
// next power of two never moves and a pair whose upper index is >= m is simply skipped.  All threads of the block take part.
__device__ __forceinline__ void add_bitonic(int64_t* a, int64_t m) {
    int64_t np2 = 1;
    while (np2 < m) np2 <<= 1;
    for (int64_t k = 2; k <= np2; k <<= 1) {
        for (int64_t j = k >> 1; j >= 1; j >>= 1) {
            for (int64_t t = threadIdx.x; t < (np2 >> 1); t += blockDim.x) {
                const int64_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // lower index of pair t
                const int64_t p = j == (k >> 1) ? (i ^ (k - 1)) : (i | j);
                if (p < m) {
                    const int64_t u = a[i], v = a[p];
                    if (u > v) { a[i] = v; a[p] = u; }
                }
            }
            __syncthreads();
        }
    }
}

// One block per list: its new segment sorted by id.  Up to ADD_SORT_LDS ids are sorted in LDS; a longer segment (a skewed add:
// every row in one list) is sorted in place in the blob by the same network -- one block, global memory, slow and correct.
constexpr int ADD_SORT_LDS = 4096;
__global__ void __launch_bounds__(1024) k_add_sort(const int64_t* __restrict__ old_off, const int64_t* __restrict__ new_off, int64_t* new_ids) {
    __shared__ int64_t buf[ADD_SORT_LDS];
    const int64_t l = blockIdx.x;
    const int64_t beg = new_off[l] + (old_off[l + 1] - old_off[l]), m = new_off[l + 1] - beg;
    if (m < 2) return;  // (uniform for the block)
    int64_t* seg = new_ids + beg;
    if (m <= ADD_SORT_LDS) {
        for (int64_t i = threadIdx.x; i < m; i += blockDim.x) buf[i] = seg[i];
        __syncthreads();
        add_bitonic(buf, m);
        for (int64_t i = threadIdx.x; i < m; i += blockDim.x) seg[i] = buf[i];
    } else {
        __syncthreads();
        add_bitonic(seg, m);
    }
}

// One wave per row of the NEW index: an old row moves up by its list's shift (id and vector), a new slot gathers the row its id names.
__global__ void __launch_bounds__(256) k_add_fill(const int64_t* __restrict__ old_off, const int64_t* __restrict__ new_off, int64_t nlist,
                                                  const int64_t* __restrict__ old_ids, const float* __restrict__ old_vecs,
                                                  const float* __restrict__ x, int64_t ntotal_old, int64_t ntotal_new, int d,
                                                  int64_t* new_ids, float* __restrict__ new_vecs) {
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (p >= ntotal_new) return;
    // the list that holds p: the largest l with new_off[l] <= p (empty lists share their offset with the next list; the largest is the non-empty one)
    int64_t lo = 0, hi = nlist;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (new_off[mid] <= p) lo = mid;
        else hi = mid;
    }
    const int64_t r = p - new_off[lo], ob = old_off[lo], olen = old_off[lo + 1] - ob;
    const float* src;
    if (r < olen) {
        src = old_vecs + (ob + r) * d;
        if (lane == 0) new_ids[p] = old_ids[ob + r];
    } else {
        src = x + (new_ids[p] - ntotal_old) * d;
    }
    float4* dst = (float4*)(new_vecs + p * d);
    for (int e = lane; e < (d >> 2); e += 64) dst[e] = ((const float4*)src)[e];
}

}  // namespace rvcmi
