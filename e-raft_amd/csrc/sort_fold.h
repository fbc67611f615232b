// sort_fold.h -- the two block-level steps splat.hip and voxel.hip share.
//
// Both files turn a scatter whose reference folds serially into a gather by a counting sort: count
// per key, exclusive scan of the counts, bucket, order each bucket, fold in key order.  The scan of
// one value per thread and the ordering of a bucket by rank are the same wherever they run; what a
// caller scans (how many counts a thread owns, a carry over super-chunks) and where a bucket's keys
// live stay with the caller.
#pragma once
#include "ecorr_device.h"

namespace ecorr {

// Exclusive scan of one value per thread over a block of NT threads (whole waves): shuffle ladder
// within the wave, the waves' sums in wsum[NT / kWave] (LDS), every thread adds the sums of the waves
// before its own.  Returns this thread's exclusive prefix; total = the block's sum, in every thread.
// Integer adds (wrapping for unsigned T): exact in any order.  Block-uniform call; ends on a
// barrier, so wsum may be reused at once.
template <int NT, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* wsum, T& total) {
    static_assert(NT % kWave == 0 && NT <= 1024, "whole 64-lane waves, wsum[NT / kWave]");
    const int lane = threadIdx.x % kWave, wv = threadIdx.x / kWave;
    T inc = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const T u = __shfl_up(inc, d, kWave);
        if (lane >= d) inc += u;
    }
    if (lane == kWave - 1) wsum[wv] = inc;
    __syncthreads();
    T pre = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < NT / kWave; ++w) {
        if (w < wv) pre += wsum[w];
        sum += wsum[w];
    }
    total = sum;
    __syncthreads();
    return pre + inc - v;
}

// Ordering a bucket by rank: the slot holding `key` goes to lo + rank_in_run(...), the number of keys
// of its run [lo, hi) smaller than it (keys of a run are distinct); key_at(j) = the key in slot j.
// hi - lo independent reads per slot, so a heavy bucket costs depth k, not the k^2 serial steps of an
// insertion sort on one thread.
template <typename K, typename KeyAt>
__device__ __forceinline__ int rank_in_run(int lo, int hi, K key, KeyAt key_at) {
    int r = 0;
    for (int j = lo; j < hi; ++j) r += key_at(j) < key;
    return r;
}

}  // namespace ecorr
