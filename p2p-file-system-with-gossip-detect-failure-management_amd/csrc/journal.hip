// Detection journal (gh_journal_*; DESIGN.md "Journal"): per member, when it
// started and stopped, when and by whom it was first detected, how often it
// was detected while running, when every view had dropped or learnt it; over
// the members, the latency histograms; per round, a log entry of sums. No
// reference counterpart (the reference logs each detection, detectfailure
// slave/slave.go:460-482, and each REMOVE it sends, Remove :338-363).
//
//   k_journal  one thread per local column, after k_finish of round r. It
//              reads what the round left behind -- det_cnt / det_min of D_r
//              (k_finish of round r + 1 is the next to clear them), alive[],
//              with GH_JOURNAL_VIEWS the census' listed[] of the new table --
//              and the member's own record, and writes that record back where
//              it changed. The round's sums: counts by ballot and popcount,
//              sums by a wave reduction, one 64-bit atomic per wave and
//              non-zero sum into the round's log entry. The histograms: LDS
//              bins per workgroup, then one global atomic per non-zero bin.
//              Everything is integer, so the order is free. Lanes past ncol
//              (the tail wave, the column padding) take part in the ballots
//              and reductions with zeros and touch no memory.
#include "gh_internal.h"

namespace {

constexpr int kBins = GH_JOURNAL_BINS;

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
  for (int w = 32; w > 0; w >>= 1) x += __shfl_xor(x, w);
  return x;
}

__global__ __launch_bounds__(256) void k_journal(GhJournal j, const int32_t* __restrict__ cnt,
                                                 const int32_t* __restrict__ dmin,
                                                 const uint8_t* __restrict__ alive,
                                                 const int32_t* __restrict__ listed, int32_t ncol, int32_t r,
                                                 int32_t running) {
  __shared__ uint32_t bins[3 * kBins];
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t c = (int64_t)blockIdx.x * 256 + tid;
  if (tid < 3 * kBins) bins[tid] = 0u;
  if (c < GH_JR_SUMS && j.next) j.next[c] = 0ull;  // (the entry after this round's: nobody adds to it yet)
  __syncthreads();

  const bool in = c < ncol;
  bool a = false;
  int32_t n = 0, L = 0;
  if (in) {
    a = alive[c] != 0;
    n = cnt[c];
    if (listed) L = listed[c];
    const bool pa = j.prev_alive[c] != 0;
    int32_t stop = j.stop_round[c], start = j.start_round[c], first = j.first_round[c];
    // 1. transitions: a start or a stop opens a new phase
    if (a != pa) {
      j.prev_alive[c] = a ? 1 : 0;
      if (a) {
        j.start_round[c] = start = r;
        if (stop >= 0) j.stop_round[c] = -1;
        stop = -1;
      } else {
        j.stop_round[c] = stop = r;
      }
      if (first >= 0) {
        j.first_round[c] = j.first_detector[c] = -1;
        j.first_count[c] = 0;
        first = -1;
      }
      if (listed) j.forgotten_round[c] = j.known_round[c] = -1;
    }
    // 2. detection
    if (n > 0) {
      j.det_rounds[c] += 1;
      j.detectors[c] += n;
      j.last_round[c] = r;
      if (a) j.fp_rounds[c] += 1;
      if (first < 0) {
        j.first_round[c] = r;
        j.first_detector[c] = dmin[c];
        j.first_count[c] = n;
        if (!a && stop >= 0) atomicAdd(&bins[min(r - stop, kBins - 1)], 1u);  // once per stop
      }
    }
    // 3. views: nobody lists a stopped member any more / everybody a running one
    if (listed) {
      if (!a && L == 0 && j.forgotten_round[c] < 0) {
        j.forgotten_round[c] = r;
        if (stop >= 0) atomicAdd(&bins[kBins + min(r - stop, kBins - 1)], 1u);
      }
      if (a && L == running - 1 && j.known_round[c] < 0) {
        j.known_round[c] = r;
        if (start >= 0) atomicAdd(&bins[2 * kBins + min(r - start, kBins - 1)], 1u);
      }
    }
  }

  // the round's log entry
  if (j.slot) {
    const bool det = n > 0;
    const uint32_t n_run = (uint32_t)__popcll(__ballot(a));
    const uint32_t n_fail = (uint32_t)__popcll(__ballot(det));
    const uint32_t n_false = (uint32_t)__popcll(__ballot(det && a));
    const uint32_t s_det = wave_sum((uint32_t)n);
    const uint32_t s_false = wave_sum(a ? (uint32_t)n : 0u);
    uint32_t s_stale = 0u, s_miss = 0u;
    if (listed) {
      s_stale = wave_sum(in && !a ? (uint32_t)L : 0u);
      s_miss = wave_sum(a ? (uint32_t)(running - 1 - L) : 0u);
    }
    if (lane == 0) {
      const uint32_t v[GH_JR_SUMS] = {n_run, n_fail, n_false, s_det, s_false, s_stale, s_miss};
#pragma unroll
      for (int x = 0; x < GH_JR_SUMS; ++x)
        if (v[x]) atomicAdd(&j.slot[x], (unsigned long long)v[x]);
    }
  }

  __syncthreads();
  if (tid < 3 * kBins && bins[tid]) atomicAdd(&j.hist[tid], (unsigned long long)bins[tid]);
}

}  // namespace

void launch_journal(const GhJournal& j, const int32_t* cnt, const int32_t* dmin, const uint8_t* alive,
                    const int32_t* listed, int32_t ncol, int32_t r, int32_t running, hipStream_t s) {
  if (ncol <= 0) return;
  hipLaunchKernelGGL(k_journal, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, s, j, cnt, dmin, alive, listed,
                     ncol, r, running);
}
