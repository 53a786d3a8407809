// File-table audit and replica selection (gh_file_audit / gh_file_select;
// DESIGN.md "File audit"): the master's replica table summarised against an
// availability set A, read-only, one lane per local file slot (file
// fl * fsh + frank, as k_repair). A is Update_metadata's `available`
// (master/master.go:93-99: the observer's present members) or the running
// processes (alive[]); a file's working count w is its slots naming a member
// of A, counted as k_repair counts them (place.hip, slots, not distinct
// members).
//
//   k_fa_bits     A and the master's list as flat bitmaps over the member ids
//                 (N / 8 bytes each: the R lookups of a file stay in 8 KB at
//                 N = 65,536), from the gathered row bitmaps (rbits) or alive[]
//   k_file_audit  per file: w, Init_replica's two preconditions
//                 (master/master.go:129-135, place.hip init_replica) for the
//                 files with w < R, the distinct members it names (load) and,
//                 when w == 1, the member its one working slot names (sole).
//                 The 11 counters are reduced in the wave (ballot + popcount),
//                 then in LDS, then by one 64-bit atomic per bin and workgroup.
//                 load / sole: int32 atomics, in LDS bins per workgroup when
//                 N <= lds_n (few members: every global atomic would land on a
//                 handful of addresses), flushed where non-zero; else global.
//   k_file_select the ids of the files matching (member, max_working), ballot-
//                 compacted per wave into an unordered list the host sorts
//                 (as gh_repair sorts its plan): GH_FS_ORDERED=0.
//   k_fs_count / k_fs_scan / k_fs_write   the same ids in ascending order
//                 without a sort (the default): every workgroup owns a
//                 contiguous range of slots, counts its matches, one workgroup
//                 scans the counts, and the ranges are walked again, each
//                 match written at its rank.
// Everything is integer, so the results do not depend on the order.
#include <algorithm>

#include "gh_internal.h"

namespace {

constexpr int kCnt = GH_AUDIT_BINS + 2;  // working_hist, files, starved
constexpr int kGridMax = 1024;           // workgroups of a launch at most (grid-stride over the slots)

__device__ __forceinline__ bool fbit(const uint32_t* b, int32_t a) { return (b[a >> 5] >> (a & 31)) & 1u; }

// qm / qo: the rbits rows of the master / the observer (nr rows gathered),
// -1 = none (no master bitmap; A = alive[]).
__global__ __launch_bounds__(256) void k_fa_bits(GhDev d, int nr, int qm, int qo, uint32_t* abits, uint32_t* mbits) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= (d.n + 31) / 32) return;
  uint32_t a = 0u, m = 0u;
  for (int b = 0; b < 32; ++b) {
    const int j = w * 32 + b;
    if (j >= d.n) break;
    a |= (uint32_t)(qo >= 0 ? gh_gbit(d, d.rbits, nr, qo, j) : d.alive[j] != 0) << b;
    if (qm >= 0) m |= (uint32_t)gh_gbit(d, d.rbits, nr, qm, j) << b;
  }
  abits[w] = a;
  if (qm >= 0) mbits[w] = m;
}

// The R slots of local file fl (contiguous, 4 R bytes) in one or two vector
// loads where R allows.
template <int R>
__device__ __forceinline__ void load_slots(const int32_t* rep, int64_t fl, int32_t (&rp)[R]) {
  const int32_t* p = rep + fl * R;
  if constexpr (R % 4 == 0) {
#pragma unroll
    for (int k = 0; k < R / 4; ++k) {
      const int4 v = reinterpret_cast<const int4*>(p)[k];
      rp[4 * k] = v.x, rp[4 * k + 1] = v.y, rp[4 * k + 2] = v.z, rp[4 * k + 3] = v.w;
    }
  } else if constexpr (R % 2 == 0) {
#pragma unroll
    for (int k = 0; k < R / 2; ++k) {
      const int2 v = reinterpret_cast<const int2*>(p)[k];
      rp[2 * k] = v.x, rp[2 * k + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < R; ++k) rp[k] = p[k];
  }
}

template <int R, bool LDS>
__global__ __launch_bounds__(256) void k_file_audit(GhDev d, GhFileAudit o) {
  __shared__ unsigned long long s_cnt[kCnt];
  __shared__ int32_t s_bins[LDS ? 2 * GH_FA_LDS_MAX : 2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int32_t n = d.n;
  int32_t* ld = LDS ? s_bins : o.load;
  int32_t* so = LDS ? s_bins + n : o.sole;
  if (tid < kCnt) s_cnt[tid] = 0ull;
  if (LDS)
    for (int x = tid; x < 2 * n; x += 256) s_bins[x] = 0;
  __syncthreads();
  // the master's candidates (Init_replica draws cand[0 .. M-2])
  const int32_t M = o.want_starved ? d.ncand[0] : 0;
  const int32_t last = M > 1 ? d.cand[M - 1] : -1;
  unsigned long long acc = 0ull;  // lane b < kCnt: counter b of this wave
  for (int64_t base = (int64_t)blockIdx.x * 256; base < d.fcap; base += (int64_t)gridDim.x * 256) {
    const int64_t fl = base + tid;
    const bool ex = fl < d.fcap && d.ver[fl] >= 0;
    int w = 0, in_pool = 0;
    if (ex) {
      int32_t rp[R];
      load_slots<R>(d.rep, fl, rp);
      int32_t one = -1;
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const int32_t a = rp[q];
        if (a < 0 || a >= n) continue;
        if (fbit(o.abits, a)) {  // :93-99
          w++;
          one = a;
          if (M > 1) in_pool += a != last && fbit(o.mbits, a);
        }
        bool first = true;  // a member named twice holds the file once
#pragma unroll
        for (int p = 0; p < q; ++p) first &= rp[p] != a;
        if (first && o.load) atomicAdd(&ld[a], 1);
      }
      if (w == 1 && o.sole) atomicAdd(&so[one], 1);
    }
    // master/master.go:129-135: Intn(M - 1) panics; the draw loop never ends
    const bool starved = ex && w < R && o.want_starved && (M <= 1 || (M - 1) - in_pool < R - w);
#pragma unroll
    for (int b = 0; b <= R; ++b) {
      const unsigned long long m = __ballot(ex && w == b);
      if (lane == b) acc += (unsigned long long)__popcll(m);
    }
    const unsigned long long me = __ballot(ex), ms = __ballot(starved);
    if (lane == GH_AUDIT_BINS) acc += (unsigned long long)__popcll(me);
    if (lane == GH_AUDIT_BINS + 1) acc += (unsigned long long)__popcll(ms);
  }
  if (lane < kCnt && acc) atomicAdd(&s_cnt[lane], acc);
  __syncthreads();
  if (tid < kCnt && s_cnt[tid]) atomicAdd(&o.cnt[tid], s_cnt[tid]);
  if (LDS)
    for (int x = tid; x < n; x += 256) {
      if (o.load && ld[x]) atomicAdd(&o.load[x], ld[x]);
      if (o.sole && so[x]) atomicAdd(&o.sole[x], so[x]);
    }
}

// Does local file fl match? max_working < 0: no condition on w (abits may be
// null).
template <int R>
__device__ __forceinline__ bool select_hit(const GhDev& d, const uint32_t* abits, int32_t member,
                                           int32_t max_working, int64_t fl) {
  if (fl >= d.fcap || d.ver[fl] < 0) return false;
  int32_t rp[R];
  load_slots<R>(d.rep, fl, rp);
  int w = 0;
  bool named = member < 0;
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const int32_t a = rp[q];
    named |= a == member;
    if (max_working >= 0 && a >= 0 && a < d.n) w += fbit(abits, a);
  }
  return named && (max_working < 0 || w <= max_working);
}

template <int R>
__global__ __launch_bounds__(256) void k_file_select(GhDev d, const uint32_t* abits, int32_t member,
                                                     int32_t max_working, int32_t* out, unsigned long long* n_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < d.fcap; base += (int64_t)gridDim.x * 256) {
    const int64_t fl = base + threadIdx.x;
    const bool hit = select_hit<R>(d, abits, member, max_working, fl);
    const unsigned long long m = __ballot(hit);
    if (!m) continue;
    unsigned long long at = 0ull;
    if (lane == 0) at = atomicAdd(n_out, (unsigned long long)__popcll(m));
    at = __shfl(at, 0);
    // (at most fcap files hit, and out holds fcap ids)
    if (hit) out[at + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)(fl * d.fsh + d.frank);
  }
}

// Ordered selection: workgroup b owns the slots [b * spb, (b + 1) * spb), spb a
// multiple of 256. Its matches -> wgc[b].
template <int R>
__global__ __launch_bounds__(256) void k_fs_count(GhDev d, const uint32_t* abits, int32_t member, int32_t max_working,
                                                  int64_t spb, uint32_t* wgc) {
  __shared__ uint32_t s_n;
  if (threadIdx.x == 0) s_n = 0u;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * spb;
  uint32_t mine = 0u;
  for (int64_t base = lo; base < lo + spb; base += 256)
    mine += (uint32_t)__popcll(__ballot(select_hit<R>(d, abits, member, max_working, base + threadIdx.x)));
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_n, mine);
  __syncthreads();
  if (threadIdx.x == 0) wgc[blockIdx.x] = s_n;
}

// wgc[0..nb) (nb <= kGridMax) -> its exclusive prefix sums, the total -> *n_out.
__global__ __launch_bounds__(kGridMax) void k_fs_scan(uint32_t* wgc, int nb, unsigned long long* n_out) {
  __shared__ uint32_t s[kGridMax];
  const int tid = threadIdx.x;
  const uint32_t own = tid < nb ? wgc[tid] : 0u;
  s[tid] = own;
  __syncthreads();
  for (int off = 1; off < kGridMax; off <<= 1) {
    const uint32_t v = tid >= off ? s[tid - off] : 0u;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  if (tid < nb) wgc[tid] = s[tid] - own;
  if (tid == kGridMax - 1) *n_out = s[tid];
}

// The workgroup's matches, in slot order, at out[wgo[b] ...].
template <int R>
__global__ __launch_bounds__(256) void k_fs_write(GhDev d, const uint32_t* abits, int32_t member, int32_t max_working,
                                                  int64_t spb, const uint32_t* wgo, int32_t* out) {
  __shared__ uint32_t s_w[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t lo = (int64_t)blockIdx.x * spb;
  uint32_t run = wgo[blockIdx.x];  // (at most fcap matches in all, and out holds fcap ids)
  for (int64_t base = lo; base < lo + spb; base += 256) {
    const int64_t fl = base + threadIdx.x;
    const bool hit = select_hit<R>(d, abits, member, max_working, fl);
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      before += x < wave ? s_w[x] : 0u;
      all += s_w[x];
    }
    if (hit) out[run + before + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)(fl * d.fsh + d.frank);
    run += all;
    __syncthreads();
  }
}

unsigned grid_for(const GhDev& d) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((d.fcap + 255) / 256, kGridMax));
}

template <int R>
void audit_r(const GhDev& d, const GhFileAudit& o, bool lds, hipStream_t s) {
  if (lds)
    hipLaunchKernelGGL((k_file_audit<R, true>), dim3(grid_for(d)), dim3(256), 0, s, d, o);
  else
    hipLaunchKernelGGL((k_file_audit<R, false>), dim3(grid_for(d)), dim3(256), 0, s, d, o);
}

template <int R>
void select_r(const GhDev& d, const uint32_t* abits, int32_t member, int32_t max_working, int32_t* out,
              unsigned long long* n_out, hipStream_t s) {
  hipLaunchKernelGGL(k_file_select<R>, dim3(grid_for(d)), dim3(256), 0, s, d, abits, member, max_working, out, n_out);
}

template <int R>
void select_ordered_r(const GhDev& d, const uint32_t* abits, int32_t member, int32_t max_working, int32_t* out,
                      unsigned long long* n_out, uint32_t* wgc, hipStream_t s) {
  const int64_t chunks = (d.fcap + 255) / 256;
  const int64_t spb = (chunks + kGridMax - 1) / kGridMax * 256;  // slots per workgroup
  const unsigned nb = (unsigned)((d.fcap + spb - 1) / spb);
  hipLaunchKernelGGL(k_fs_count<R>, dim3(nb), dim3(256), 0, s, d, abits, member, max_working, spb, wgc);
  hipLaunchKernelGGL(k_fs_scan, dim3(1), dim3(kGridMax), 0, s, wgc, (int)nb, n_out);
  hipLaunchKernelGGL(k_fs_write<R>, dim3(nb), dim3(256), 0, s, d, abits, member, max_working, spb, wgc, out);
}

}  // namespace

void launch_fa_bits(const GhDev& d, int nr, int qm, int qo, uint32_t* abits, uint32_t* mbits, hipStream_t s) {
  const int nw = (d.n + 31) / 32;
  hipLaunchKernelGGL(k_fa_bits, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, d, nr, qm, qo, abits, mbits);
}

#define GH_FOR_R(R, CALL) \
  switch (R) {            \
    case 1: CALL(1); break; \
    case 2: CALL(2); break; \
    case 3: CALL(3); break; \
    case 4: CALL(4); break; \
    case 5: CALL(5); break; \
    case 6: CALL(6); break; \
    case 7: CALL(7); break; \
    case 8: CALL(8); break; \
  }

void launch_file_audit(const GhDev& d, int32_t R, const GhFileAudit& o, int32_t lds_n, hipStream_t s) {
  if (d.fcap <= 0) return;
  const bool lds = d.n <= std::min<int32_t>(lds_n, GH_FA_LDS_MAX);
#define GH_CALL(r) audit_r<r>(d, o, lds, s)
  GH_FOR_R(R, GH_CALL)
#undef GH_CALL
}

void launch_file_select(const GhDev& d, int32_t R, const uint32_t* abits, int32_t member, int32_t max_working,
                        int32_t* out, unsigned long long* n_out, uint32_t* wgc, hipStream_t s) {
  if (d.fcap <= 0) return;
  if (wgc) {
#define GH_CALL(r) select_ordered_r<r>(d, abits, member, max_working, out, n_out, wgc, s)
    GH_FOR_R(R, GH_CALL)
#undef GH_CALL
    return;
  }
#define GH_CALL(r) select_r<r>(d, abits, member, max_working, out, n_out, s)
  GH_FOR_R(R, GH_CALL)
#undef GH_CALL
}
