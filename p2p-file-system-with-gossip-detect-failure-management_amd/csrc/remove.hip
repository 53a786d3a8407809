// The reference's REMOVE recipients (GH_REMOVE_LIST; one engine, member-ID
// list order).
//
// detectfailure (slave/slave.go:460-482) calls removeMember(c) and then
// Remove(c) (:472-473) for each member it detects, in list order, and Remove
// messages every member of the detector's list as it stands at that moment,
// itself excluded (:338-363, :344-346). So row j receives REMOVE(c) in round
// r + 1 iff some row i that detected c in round r listed j when it did:
//
//   R(j, c) = exists i in det(c): listed_i(j) and not (det_i(j) and j <= c)
//
// (listed_i = the row's list before the sweep: present after step 1's
// REMOVEs, self excluded; det_i = the members the sweep removed; in ID order
// the ones removed before c are those below it, and c itself). Split by j:
//
//   j <  c: det(c) meets surv(j) = {i : listed_i(j), not det_i(j)}
//   j >  c: det(c) meets lst(j)  = {i : listed_i(j)}
//   j == c: never (c is gone from every detector's list)
//
// k_rm_cols builds, over the rows that ran the sweep, the column bitmaps
// det(x), surv(x), lst(x) and the counts |surv(x)|, |lst(x)| in one pass over
// the round's input table; k_rm_recv decides every (j, c) of D_r from the
// counts (an empty set: no; |det(c)| + |set| > rows: yes, by pigeonhole) and
// intersects the two bitmaps only where neither settles it (detection storms).
// A healthy cluster's crash wave needs no intersection at all: every row
// detects a crashed member, and a live receiver survives in every list.
#include <limits.h>

#include "gh_internal.h"

namespace {

// Any detection in this round (D_r non-empty): ccnt[2 ld + 1]
__global__ __launch_bounds__(256) void k_rm_any(GhDev d, int dnew, GhRound p) {
  int any = 0;
  for (int64_t x = threadIdx.x; x < p.ld; x += 256) any |= d.det_cnt[dnew][x] > 0;
  if (__syncthreads_or(any) && threadIdx.x == 0) d.ccnt[2 * p.ld + 1] = 1;
}

// One workgroup per 256 local columns x 256 rows: thread (chunk k, group g)
// reads 8 columns of 32 rows and writes their 24 bitmap words. DET_ONLY (an
// engine armed by gh_set_partition): det(x) alone, the 8 words of cdet; csurv,
// clst and the counts are not allocated there.
template <bool DET_ONLY>
__global__ __launch_bounds__(256) void k_rm_cols(GhDev d, int cur, int dcur, GhRound p) {
  if (d.ccnt[2 * p.ld + 1] == 0) return;
  __shared__ int s_surv[256], s_lst[256], s_rows;
  const int nrb = (int)((p.n + 255) / 256);
  const int cb = blockIdx.x / nrb, rb = blockIdx.x - cb * nrb;
  const int k = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int64_t c = (int64_t)cb * 256 + 8 * k;
  s_surv[threadIdx.x] = 0;
  s_lst[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_rows = 0;
  __syncthreads();
  uint32_t wd[8] = {}, ws[8] = {}, wl[8] = {};
  const int64_t i0 = (int64_t)rb * 256 + 32 * g;
  int rows = 0;
  if (c < p.ld) {
    const uint32_t b8 = (d.dbits[c >> 5] >> (c & 31)) & 0xFFu;  // D_{r-1} in these columns
    const bool tier = gh_m8(d, cur);
    // 8 rows at a time, their plane and age words loaded together: a tier
    // chunk's present cells are its codes other than 15 (it holds no flag),
    // only escaped chunks decode their 16-bit codes
    for (int q0 = 0; q0 < 32; q0 += 8) {
      uint32_t pw[8], aw[8];
      uint8_t act[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int64_t i = i0 + q0 + u;
        act[u] = i < p.n ? d.active[i] : 0;
        pw[u] = aw[u] = 0;
        if (tier && i < p.n) {
          const int64_t cell = gh_cell(d, i, c);
          aw[u] = d.a4[cur][cell >> 3];
          pw[u] = d.pl[cur][cell >> 3];
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int q = q0 + u;
        const int64_t i = i0 + q;
        if (!act[u]) continue;
        rows++;
        uint32_t pf;
        if (tier && !gh_t4_esc(aw[u])) {
          const uint32_t n15 = ~pw[u];  // a nibble of 15 is absent or a tombstone
          uint32_t t = n15 | (n15 >> 2);
          t |= t >> 1;
          pf = 0;
#pragma unroll
          for (int j = 0; j < 8; ++j) pf |= ((t >> gh_nib(j)) & 1u) << j;
        } else {
          pf = gh_pf8(d, cur, i, c);
        }
        uint32_t lst = pf & 0xFFu;
        for (uint32_t m = lst & b8; m; m &= m - 1) {  // step 1: REMOVE'd at row i
          const int j = __builtin_ctz(m);
          if (gh_rm_at(d, dcur, c + j, i)) lst &= ~(1u << j);
        }
        if (i >= c && i < c + 8) lst &= ~(1u << (i - c));  // Remove skips self (:344-346)
        const uint32_t det = (pf >> 8) & lst;              // the sweep's removals
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          wd[j] |= ((det >> j) & 1u) << q;
          ws[j] |= ((lst & ~det) >> j & 1u) << q;
          wl[j] |= ((lst >> j) & 1u) << q;
        }
      }
    }
    const int64_t w = i0 >> 5;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (c + j >= p.ld) break;
      const int64_t o = (c + j) * d.nw + w;
      if (w < d.nw) {
        d.cdet[o] = wd[j];
        if constexpr (!DET_ONLY) {
          d.csurv[o] = ws[j];
          d.clst[o] = wl[j];
        }
      }
      if constexpr (!DET_ONLY) {
        atomicAdd(&s_surv[8 * k + j], __popc(ws[j]));
        atomicAdd(&s_lst[8 * k + j], __popc(wl[j]));
      }
    }
  }
  if constexpr (DET_ONLY) return;  // (no barrier below is skipped by part of a workgroup: all return here)
  if (k == 0 && cb == 0) atomicAdd(&s_rows, rows);
  __syncthreads();
  const int64_t cc = (int64_t)cb * 256 + threadIdx.x;
  if (cc < p.ld) {
    if (s_surv[threadIdx.x]) atomicAdd(&d.ccnt[cc], s_surv[threadIdx.x]);
    if (s_lst[threadIdx.x]) atomicAdd(&d.ccnt[p.ld + cc], s_lst[threadIdx.x]);
  }
  if (threadIdx.x == 0 && cb == 0 && s_rows) atomicAdd(&d.ccnt[2 * p.ld], s_rows);
}

__device__ __forceinline__ bool meets(const uint32_t* a, const uint32_t* b, int64_t nw) {
  for (int64_t w = 0; w < nw; ++w)
    if (a[w] & b[w]) return true;
  return false;
}

// One workgroup per member c of D_r (grid-stride), a thread per 32 receivers.
// The nonzero words of det(c) are listed in LDS first, so an intersection
// costs one word per listed word (at most |det(c)|), not N / 32: a member
// with few detectors (the common case outside storms, where counts and the
// pigeonhole rule settle most pairs) is decided in O(|det(c)|) per receiver.
constexpr int RM_NZ_CAP = 2048;  // listed words (nw <= 2048 up to N = 65,536; beyond: the full scan)
__global__ __launch_bounds__(256) void k_rm_recv(GhDev d, int dnew, GhRound p) {
  __shared__ uint32_t s_w[RM_NZ_CAP], s_v[RM_NZ_CAP];
  __shared__ int s_nz;
  const int nd = d.nd[2 + dnew];
  const int nact = d.ccnt[2 * p.ld];
  for (int q = blockIdx.x; q < nd; q += gridDim.x) {
    const int64_t c = d.dlist[(int64_t)dnew * p.ld + q];
    const int detc = d.det_cnt[dnew][c];
    const uint32_t* dcol = d.cdet + c * d.nw;
    if (threadIdx.x == 0) s_nz = 0;
    __syncthreads();
    for (int64_t w = threadIdx.x; w < d.nw; w += 256) {
      const uint32_t v = dcol[w];
      if (v) {
        const int at = atomicAdd(&s_nz, 1);
        if (at < RM_NZ_CAP) {
          s_w[at] = (uint32_t)w;
          s_v[at] = v;
        }
      }
    }
    __syncthreads();
    const int nz = s_nz;
    for (int64_t w = threadIdx.x; w < d.nw; w += 256) {
      uint32_t out = 0;
      for (int b = 0; b < 32; ++b) {
        const int64_t j = 32 * w + b;
        if (j >= p.n || j == c) continue;
        const bool low = j < c;
        const int cnt = low ? d.ccnt[j] : d.ccnt[p.ld + j];
        bool r = false;
        if (cnt == 0) {
          r = false;
        } else if (detc + cnt > nact) {
          r = true;  // pigeonhole: both sets live in the rows that ran the sweep
        } else {
          const uint32_t* other = (low ? d.csurv : d.clst) + j * d.nw;
          if (nz <= RM_NZ_CAP) {
            for (int e = 0; e < nz && !r; ++e) r = (s_v[e] & other[s_w[e]]) != 0u;
          } else {
            r = meets(dcol, other, d.nw);
          }
        }
        out |= (uint32_t)r << b;
      }
      d.rcv[dnew][c * d.nw + w] = out;
    }
    __syncthreads();  // s_nz / the list before the next member
  }
}

// ---- network partition (gh_set_partition; SPEC §2 step 6b) ----------------
// REMOVE(c) of D_r goes from each detector to the rows of its own side, itself
// excluded: with n_j(c) = the detectors of c on row j's side and m_j(c) the
// lowest of them, row j receives it iff n_j(c) > 0 and not (n_j(c) == 1 and
// m_j(c) == j) -- rule D4 per side. One workgroup per member c of D_r
// (grid-stride): pass 1 walks the set bits of det(c) (cdet, this round's
// sweep) into a count and a minimum per side in LDS; pass 2 writes
// rcv[dnew][c], a word per 32 receivers. Rows at or past n get no bit; side[]
// is read below n only.
__global__ __launch_bounds__(256) void k_part_recv(GhDev d, int dnew, GhRound p) {
  __shared__ int s_cnt[GH_PART_SIDES], s_min[GH_PART_SIDES];
  const int nd = d.nd[2 + dnew];
  for (int q = blockIdx.x; q < nd; q += gridDim.x) {
    const int64_t c = d.dlist[(int64_t)dnew * p.ld + q];
    if (c < 0 || c >= d.ncol) continue;  // (a padded column is never detected; uniform)
    if (threadIdx.x < GH_PART_SIDES) {
      s_cnt[threadIdx.x] = 0;
      s_min[threadIdx.x] = INT_MAX;
    }
    __syncthreads();
    const uint32_t* dcol = d.cdet + c * d.nw;
    for (int64_t w = threadIdx.x; w < d.nw; w += 256) {
      for (uint32_t v = dcol[w]; v; v &= v - 1u) {
        const int64_t i = 32 * w + __builtin_ctz(v);
        if (i >= p.n) break;
        const int sd = d.side[i] & (GH_PART_SIDES - 1);
        atomicAdd(&s_cnt[sd], 1);
        atomicMin(&s_min[sd], (int)i);
      }
    }
    __syncthreads();
    for (int64_t w = threadIdx.x; w < d.nw; w += 256) {
      uint32_t out = 0;
      for (int b = 0; b < 32; ++b) {
        const int64_t j = 32 * w + b;
        if (j >= p.n) break;
        const int sd = d.side[j] & (GH_PART_SIDES - 1);
        const int nj = s_cnt[sd];
        out |= (uint32_t)(nj > 0 && !(nj == 1 && s_min[sd] == j)) << b;
      }
      d.rcv[dnew][c * d.nw + w] = out;
    }
    __syncthreads();  // the LDS tables before the next member
  }
}

// On arming while a REMOVE set is pending (parity dcur, detected before any
// side existed): its recipients by rule D4 -- every row below n but a sole
// detector.
__global__ __launch_bounds__(256) void k_part_fill(GhDev d, int dcur, GhRound p) {
  const int nd = d.nd[2 + dcur];
  for (int q = blockIdx.x; q < nd; q += gridDim.x) {
    const int64_t c = d.dlist[(int64_t)dcur * p.ld + q];
    if (c < 0 || c >= d.ncol) continue;
    const int64_t sole = d.det_cnt[dcur][c] == 1 ? d.det_min[dcur][c] : -1;
    for (int64_t w = threadIdx.x; w < d.nw; w += 256) {
      const int64_t left = p.n - 32 * w;  // rows of this word below n (>= 1)
      uint32_t out = left >= 32 ? 0xFFFFFFFFu : (1u << left) - 1u;
      if (sole >= 32 * w && sole < 32 * w + 32) out &= ~(1u << (sole & 31));
      d.rcv[dcur][c * d.nw + w] = out;
    }
  }
}

// ---- lossy control messages (gh_set_control_loss, GH_CTL_REMOVE; SPEC §2
// step 6c) --------------------------------------------------------------------
// REMOVE(c) of D_r is one message per (detector i, row j), i != j and reach(i,
// j), dropped by Philox(K; i, j, 'CRMV', 0) under the key K = words 0, 1 of
// W('CRMV'; c, r, 0) against out[i] and in[j]; row j receives it iff one of
// them arrives. One workgroup per member c of D_r (grid-stride): K once per
// workgroup, the nonzero words of det(c) listed in LDS as in k_rm_recv (past
// the cap: the full scan of det(c)), then a thread per 32 receivers, each
// walking the detectors until the first message that arrives: at rate p an
// expected 1 / (1 - p^2) draws per pair. The words are walked in the order
// they were listed, which is not ascending and varies from run to run; only
// the number of draws depends on it, every message's fate being a pure
// function of its counter. in[j] == always settles a receiver
// and out[i] == always skips a detector without a draw, and so do two zero
// thresholds. SIDES = false: the host knows every member is on one side.
// Counters (ctl[0] pairs with a message and j alive, ctl[1] those with every
// message dropped): reduced per workgroup, one atomic each. Rows at or past n
// get no bit; the thresholds and side[] are read below n only.
struct CtlWalk {
  uint64_t key;
  const uint32_t* out;
  uint32_t tin;
  int64_t j;
  bool has, got;
  // the detectors of word w (bits v): true when the walk is over
  template <bool SIDES>
  __device__ __forceinline__ bool word(const int32_t* sd, int64_t w, uint32_t v, int32_t n) {
    for (; v; v &= v - 1u) {
      const int64_t i = 32 * w + __builtin_ctz(v);
      if (i >= n) break;
      if (i == j) continue;  // Remove skips self (:344-346)
      if (SIDES && sd[i] != sd[j]) continue;
      has = true;
      if (tin == GH_LOSS_ALWAYS) return true;
      const uint32_t to = out[i];
      if (to == GH_LOSS_ALWAYS) continue;
      if ((to | tin) == 0u) return got = true;
      uint32_t b[4];
      gh_philox_block(key, (uint32_t)i, (uint32_t)j, GH_TAG_CRMV, 0u, b);
      if (!(b[0] < to || b[1] < tin)) return got = true;
    }
    return false;
  }
};

template <bool SIDES>
__global__ __launch_bounds__(256) void k_ctl_recv(GhDev d, int dnew, GhRound p) {
  __shared__ uint32_t s_w[RM_NZ_CAP], s_v[RM_NZ_CAP];
  __shared__ int s_nz, s_tot[2];
  const int nd = d.nd[2 + dnew];
  const uint32_t* thr = d.link + 4;
  if (threadIdx.x < 2) s_tot[threadIdx.x] = 0;
  int pairs = 0, missed = 0;
  for (int q = blockIdx.x; q < nd; q += gridDim.x) {
    const int64_t c = d.dlist[(int64_t)dnew * p.ld + q];
    if (c < 0 || c >= d.ncol) continue;  // (a padded column is never detected; uniform)
    uint32_t kw[4];
    gh_philox_block(p.seed, (uint32_t)c, (uint32_t)p.r, GH_TAG_CRMV, 0u, kw);
    const uint32_t* dcol = d.cdet + c * d.nw;
    if (threadIdx.x == 0) s_nz = 0;
    __syncthreads();
    for (int64_t w = threadIdx.x; w < d.nw; w += 256) {
      const uint32_t v = dcol[w];
      if (v) {
        const int at = atomicAdd(&s_nz, 1);
        if (at < RM_NZ_CAP) {
          s_w[at] = (uint32_t)w;
          s_v[at] = v;
        }
      }
    }
    __syncthreads();
    const int nz = s_nz;
    for (int64_t w = threadIdx.x; w < d.nw; w += 256) {
      uint32_t out = 0;
      for (int b = 0; b < 32; ++b) {
        const int64_t j = 32 * w + b;
        if (j >= p.n) break;
        CtlWalk k{(uint64_t)kw[0] | ((uint64_t)kw[1] << 32), thr, thr[p.n + j], j, false, false};
        if (nz <= RM_NZ_CAP) {
          for (int e = 0; e < nz; ++e)
            if (k.word<SIDES>(d.side, s_w[e], s_v[e], p.n)) break;
        } else {
          for (int64_t x = 0; x < d.nw; ++x)
            if (k.word<SIDES>(d.side, x, dcol[x], p.n)) break;
        }
        out |= (uint32_t)k.got << b;
        const bool cnt = k.has && d.alive[j];
        pairs += cnt;
        missed += cnt && !k.got;
      }
      d.rcv[dnew][c * d.nw + w] = out;
    }
    __syncthreads();  // s_nz / the list before the next member
  }
  for (int o = 32; o > 0; o >>= 1) {
    pairs += __shfl_xor(pairs, o);
    missed += __shfl_xor(missed, o);
  }
  __syncthreads();  // (s_tot zeroed; every thread reaches this)
  if ((threadIdx.x & 63) == 0 && pairs) {
    atomicAdd(&s_tot[0], pairs);
    if (missed) atomicAdd(&s_tot[1], missed);
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_tot[threadIdx.x]) atomicAdd(&d.ctl[threadIdx.x], (unsigned long long)s_tot[threadIdx.x]);
}

}  // namespace

void launch_ctl_recv(const GhDev& d, int dnew, const GhRound& p, int one_side, hipStream_t s) {
  const dim3 grid((unsigned)std::min<int64_t>(4096, std::max<int64_t>(1, p.n)));
  if (one_side)
    hipLaunchKernelGGL(k_ctl_recv<false>, grid, dim3(256), 0, s, d, dnew, p);
  else
    hipLaunchKernelGGL(k_ctl_recv<true>, grid, dim3(256), 0, s, d, dnew, p);
}

void launch_part_cols(const GhDev& d, int cur, int dcur, const GhRound& p, hipStream_t s) {
  (void)hipMemsetAsync(d.ccnt, 0, sizeof(int32_t) * (2 * p.ld + 2), s);
  hipLaunchKernelGGL(k_rm_any, dim3(1), dim3(256), 0, s, d, dcur ^ 1, p);
  const int64_t nrb = (p.n + 255) / 256;
  hipLaunchKernelGGL(k_rm_cols<true>, dim3((unsigned)(((p.ld + 255) / 256) * nrb)), dim3(256), 0, s, d, cur, dcur, p);
}

void launch_part_recv(const GhDev& d, int dnew, const GhRound& p, hipStream_t s) {
  hipLaunchKernelGGL(k_part_recv, dim3((unsigned)std::min<int64_t>(4096, std::max<int64_t>(1, p.n))), dim3(256), 0, s, d,
                     dnew, p);
}

void launch_part_fill(const GhDev& d, int dcur, const GhRound& p, hipStream_t s) {
  hipLaunchKernelGGL(k_part_fill, dim3((unsigned)std::min<int64_t>(4096, std::max<int64_t>(1, p.n))), dim3(256), 0, s, d,
                     dcur, p);
}

void launch_rm_cols(const GhDev& d, int cur, int dcur, const GhRound& p, hipStream_t s) {
  (void)hipMemsetAsync(d.ccnt, 0, sizeof(int32_t) * (2 * p.ld + 2), s);
  hipLaunchKernelGGL(k_rm_any, dim3(1), dim3(256), 0, s, d, dcur ^ 1, p);
  const int64_t nrb = (p.n + 255) / 256;
  hipLaunchKernelGGL(k_rm_cols<false>, dim3((unsigned)(((p.ld + 255) / 256) * nrb)), dim3(256), 0, s, d, cur, dcur, p);
}

void launch_rm_recv(const GhDev& d, int dnew, const GhRound& p, hipStream_t s) {
  hipLaunchKernelGGL(k_rm_recv, dim3((unsigned)std::min<int64_t>(4096, std::max<int64_t>(1, p.n))), dim3(256), 0, s, d,
                     dnew, p);
}
