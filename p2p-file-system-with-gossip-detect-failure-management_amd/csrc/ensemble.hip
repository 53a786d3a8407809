// Cluster ensembles (gh_ens_step; SPEC §11, DESIGN.md "Ensemble"): B
// independent clusters of N <= 128 members, ONE WORKGROUP PER CLUSTER. A
// workgroup loads its cluster's tables, runs every round of the call out of
// registers and LDS with no launch per round, and stores the state once.
//
// Ownership. The kernel is compiled per size bucket NM (16, 32, 64, 128 >= N):
// 8 * NM threads, thread tid owns member column c = tid % NM of the rows
// i = 8 j + tid / NM, j < NM / 8, and keeps those cells' exact (hb, ts) IN
// REGISTERS for the whole call (2 * NM / 8 registers). Cells outside N x N are
// absent and inert: their rows are not alive, their columns are never
// detected, drawn or stored.
//
// LDS holds only what other threads read: the round's SNAPSHOT snap[NM + 1][NM]
// (the table after steps 1-5, row NM all absent: the "sender" of an invalid
// draw, so the merge has no branch), the per-row present counts, alive /
// active bytes, the two REMOVE sets (pending D_{r-1} and the D_r being built),
// each receiver's k drawn peers and the ones whose message arrived, and the
// cluster's loss thresholds. A wave's lanes read snap[p][c..c+63]: contiguous
// dwords, no bank conflict.
//
// The merge hazard (a receiver reading a sender row that was already merged
// into) cannot occur: the merge writes registers only. The snapshot is
// rewritten by the NEXT round's phase B, behind that round's barrier A, which
// every thread passes only after its merge reads of this round.
//
// One round, four barriers:
//   A  tid < N: the row's k peers (Philox 'PEER', gh_philox_block).
//      every cell: REMOVE delivery of D_{r-1} (step 1); rows count their
//      present cells (wave ballot + one LDS atomic per row and wave).
//   B  every cell: guard (step 2), own heartbeat (3), detect (4: LDS atomics
//      build D_r), clean (5); the cell goes to the snapshot.
//   C  thread (i, t): draw t of receiver i is a message iff its peer p is
//      alive, active and lists i; lost under step 6a's rule ('LINK' block, only
//      drawn when the cluster has a non-zero threshold). tid < N: member tid's
//      detect record and the round's failed / false-positive counts; the
//      consumed REMOVE set and the row counts are reset.
//   D  every cell: max over the arrived senders' snapshot rows (step 6).
#include "ensemble.h"
#include "gh_internal.h"

namespace {

enum {  // gh_ens_stats as int64 [GH_ENS_NSTAT]
  ES_ROUNDS = 0,
  ES_LAST_ROUND,
  ES_DETECTIONS,
  ES_FAILED,
  ES_REMOVE_UNKNOWN,
  ES_RING_EMPTY,
  ES_ACTIVE_ROWS,
  ES_MERGED,
  ES_RELEASED,
  ES_TOMBSTONED,
  ES_FALSE_FAILED,
  ES_FALSE_DETECTIONS,
  ES_SENT,
  ES_DROPPED
};

template <int NM>
struct EnsLds {
  static constexpr size_t st = 0;                                      // u64 [GH_ENS_NSTAT]
  static constexpr size_t snap = st + 8 * 16;                          // i32 [NM + 1][NM]
  static constexpr size_t cnt = snap + sizeof(int32_t) * (NM + 1) * NM;  // i32 [NM]
  static constexpr size_t dcnt = cnt + 4 * NM;                         // i32 [2][NM]
  static constexpr size_t dmin = dcnt + 8 * NM;                        // i32 [2][NM]
  static constexpr size_t out = dmin + 8 * NM;                         // u32 [NM]
  static constexpr size_t in = out + 4 * NM;                           // u32 [NM]
  static constexpr size_t pk = in + 4 * NM;                            // u8 [NM][8] arrived senders (NM: none)
  static constexpr size_t peer = pk + 8 * NM;                          // u8 [NM][8] drawn peers
  static constexpr size_t alive = peer + 8 * NM;                       // u8 [NM]
  static constexpr size_t active = alive + NM;                         // u8 [NM]
  static constexpr size_t bytes = active + NM;
};

__device__ __forceinline__ void ens_add(unsigned long long* st, int f, uint32_t v) {
  if (v) atomicAdd(st + f, (unsigned long long)v);
}

template <int NM>
__global__ __launch_bounds__(8 * NM) void k_ens_step(GhEns d, int32_t rounds) {
  constexpr int CPT = NM / 8;  // rows (cells) per thread
  constexpr int RW = NM < 64 ? NM : 64;  // lanes of a wave in one row
  using L = EnsLds<NM>;
  extern __shared__ __align__(16) unsigned char lds[];
  unsigned long long* s_st = reinterpret_cast<unsigned long long*>(lds + L::st);
  int32_t* s_snap = reinterpret_cast<int32_t*>(lds + L::snap);
  int32_t* s_cnt = reinterpret_cast<int32_t*>(lds + L::cnt);
  int32_t* s_dcnt = reinterpret_cast<int32_t*>(lds + L::dcnt);
  int32_t* s_dmin = reinterpret_cast<int32_t*>(lds + L::dmin);
  uint32_t* s_out = reinterpret_cast<uint32_t*>(lds + L::out);
  uint32_t* s_in = reinterpret_cast<uint32_t*>(lds + L::in);
  uint8_t* s_pk = lds + L::pk;
  uint8_t* s_peer = lds + L::peer;
  uint8_t* s_alive = lds + L::alive;
  uint8_t* s_active = lds + L::active;

  const int tid = threadIdx.x;
  const int n = d.n, k = d.k;
  const int c = tid % NM, ro = tid / NM;  // this thread's column, and its row within each group of 8
  const int lane = tid & 63;
  // the lanes of this thread's row in its wave
  const unsigned long long rowmask = RW == 64 ? ~0ull : ((1ull << RW) - 1ull) << ((lane / RW) * RW);
  const int li = tid >> 3, lt = tid & 7;  // phase C: receiver and draw

  for (int64_t b = blockIdx.x; b < d.nb; b += gridDim.x) {
    const gh_ens_params par = d.par[b];
    const int32_t r0 = d.round[b];
    const int64_t vb = b * n;  // the cluster's per-member vectors
    // ---- load ---------------------------------------------------------------
    __syncthreads();  // (the previous cluster's LDS is done with)
    int32_t my_first = -1, my_fp = 0;
    int lossy = 0;
    if (tid < NM) {
      const bool in_n = tid < n;
      s_alive[tid] = in_n ? (uint8_t)(d.alive[vb + tid] && !d.crashq[vb + tid]) : 0;  // step 0
      s_active[tid] = 0;
      s_cnt[tid] = 0;
      s_dcnt[tid] = in_n ? d.det_cnt[vb + tid] : 0;
      s_dmin[tid] = in_n ? d.det_min[vb + tid] : n;
      s_dcnt[NM + tid] = 0;
      s_dmin[NM + tid] = n;
      const uint32_t o = in_n ? d.out[vb + tid] : 0u, q = in_n ? d.in[vb + tid] : 0u;
      s_out[tid] = o;
      s_in[tid] = q;
      lossy = (o | q) != 0u;
      s_snap[NM * NM + tid] = GH_ABSENT;
      if (in_n) {
        my_first = d.first[vb + tid];
        my_fp = d.fp[vb + tid];
      }
    }
    if (tid < 16) s_st[tid] = 0;
    int32_t hb[CPT], ts[CPT];
    // (a uniform row-group base and one lane offset: no address per cell is kept)
    const int g0 = ro * n + c;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      const int64_t grp = b * n * n + (int64_t)8 * j * n;
      const bool in_n = 8 * j + ro < n && c < n;
      hb[j] = in_n ? (d.hb + grp)[g0] : GH_ABSENT;
      ts[j] = in_n ? (d.ts + grp)[g0] : 0;
    }
    lossy = __syncthreads_or(lossy);
    uint32_t amask = 0;  // bit j: row 8 j + ro is running
#pragma unroll
    for (int j = 0; j < CPT; ++j) amask |= (uint32_t)(s_alive[8 * j + ro] != 0) << j;
    const bool li_runs = lt < k && li < n && s_alive[li];
    const bool me_runs = tid < n && s_alive[tid];

    uint32_t c_tomb = 0, c_unk = 0, c_det = 0, c_rel = 0, c_mrg = 0, c_act = 0;
    uint32_t c_failed = 0, c_ff = 0, c_fd = 0, c_sent = 0, c_drop = 0;
    int pb = 0;  // the REMOVE set pending this round

    for (int32_t q = 0; q < rounds; ++q) {
      const int32_t r = r0 + 1 + q;
      // r >= 1 and T >= 0: r - T fits an int32
      const int32_t r_fail = r - par.t_fail, r_clean = r - par.t_cleanup;
      // ---- phase A: peers; REMOVE delivery (step 1); row counts ---------------
      if (me_runs) {
        for (int blk = 0; 4 * blk < k; ++blk) {
          uint32_t w[4];
          gh_philox_block(par.seed, (uint32_t)tid, (uint32_t)r, GH_TAG_PEER, (uint32_t)blk, w);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const uint32_t x = (uint32_t)(((uint64_t)w[u] * (uint64_t)(n - 1)) >> 32);
            if (4 * blk + u < k) s_peer[8 * tid + 4 * blk + u] = (uint8_t)(x + (x >= (uint32_t)tid));
          }
        }
      }
      {
        const int32_t dc = s_dcnt[pb * NM + c], dm = s_dmin[pb * NM + c];
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
          if (8 * j >= n) continue;  // (uniform: rows outside N)
          const int i = 8 * j + ro;
          // every running row but a sole detector (it removed the member itself)
          if (dc > 0 && ((amask >> j) & 1u) && !(dc == 1 && dm == i)) {
            if (hb[j] >= 0) {
              hb[j] = GH_TOMBSTONE;
              ++c_tomb;
            } else if (hb[j] == GH_ABSENT) {
              ++c_unk;
            }
          }
          const unsigned long long pres = __ballot(hb[j] >= 0) & rowmask;
          if ((lane & (RW - 1)) == 0 && pres) atomicAdd(&s_cnt[i], __popcll(pres));
        }
      }
      __syncthreads();
      // ---- phase B: guard, own heartbeat, detect, clean (steps 2-5); snapshot --
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        if (8 * j >= n) continue;  // (uniform: rows outside N)
        const int i = 8 * j + ro;
        const bool run = (amask >> j) & 1u;
        const bool act = run && s_cnt[i] >= d.min_members;
        if (run && !act) {
          if (hb[j] >= 0) ts[j] = r;  // the <4 guard: the row only stamps its list
        } else if (act) {
          if (c == i) {
            if (hb[j] >= 0) {
              ++hb[j];
              ts[j] = r;
            }
          } else if (hb[j] > 1 && ts[j] < r_fail) {
            hb[j] = GH_TOMBSTONE;
            ++c_det;
            atomicAdd(&s_dcnt[(pb ^ 1) * NM + c], 1);
            atomicMin(&s_dmin[(pb ^ 1) * NM + c], i);
          }
          if (hb[j] == GH_TOMBSTONE && ts[j] < r_clean) {
            hb[j] = GH_ABSENT;
            ++c_rel;
          }
        }
        s_snap[8 * NM * j + tid] = hb[j];  // (= [i][c]: tid = ro * NM + c)
        if (c == 0) {
          s_active[i] = act;
          c_act += act;
        }
      }
      __syncthreads();
      // ---- phase C: which draws arrive (step 6a); the round's record ----------
      {
        int s = NM;  // no sender
        if (li_runs) {
          const int p = s_peer[8 * li + lt];
          if (s_alive[p] && s_active[p] && s_snap[p * NM + li] >= 0) {
            ++c_sent;
            bool lost = false;
            if (lossy) {
              uint32_t w[4];
              gh_philox_block(par.seed, (uint32_t)li, (uint32_t)r, GH_TAG_LINK, (uint32_t)lt, w);
              lost = gh_link_hit(s_out[p], w[0]) || gh_link_hit(s_in[li], w[1]);
            }
            if (lost)
              ++c_drop;
            else
              s = p;
          }
        }
        s_pk[tid] = (uint8_t)s;  // (tid = 8 li + lt)
      }
      if (tid < NM) {
        const int32_t dn = s_dcnt[(pb ^ 1) * NM + tid];
        if (dn > 0) {
          ++c_failed;
          if (s_alive[tid]) {
            ++c_ff;
            c_fd += (uint32_t)dn;
            ++my_fp;
          } else if (my_first < 0) {
            my_first = r;
          }
        }
        s_cnt[tid] = 0;
        s_dcnt[pb * NM + tid] = 0;
        s_dmin[pb * NM + tid] = n;
      }
      __syncthreads();
      // ---- phase D: merge (step 6), into registers ----------------------------
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        if (8 * j >= n) continue;  // (uniform: rows outside N)
        const unsigned long long snd = reinterpret_cast<const unsigned long long*>(s_pk)[8 * j + ro];
        int32_t m = GH_ABSENT;
        for (int t = 0; t < k; ++t) m = max(m, s_snap[(int)((snd >> (8 * t)) & 0xFFu) * NM + c]);
        if (hb[j] >= GH_ABSENT && m > hb[j]) {
          hb[j] = m;
          ts[j] = r;
          ++c_mrg;
        }
      }
      pb ^= 1;
      // (no barrier: the next round writes s_peer and s_cnt, which phase D does
      // not read, and reaches the snapshot and s_pk only behind its barrier A)
    }

    // ---- store ----------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
      const int64_t grp = b * n * n + (int64_t)8 * j * n;
      if (8 * j + ro < n && c < n) {
        (d.hb + grp)[g0] = hb[j];
        (d.ts + grp)[g0] = ts[j];
      }
    }
    ens_add(s_st, ES_TOMBSTONED, c_tomb);
    ens_add(s_st, ES_REMOVE_UNKNOWN, c_unk);
    ens_add(s_st, ES_DETECTIONS, c_det);
    ens_add(s_st, ES_RELEASED, c_rel);
    ens_add(s_st, ES_MERGED, c_mrg);
    ens_add(s_st, ES_ACTIVE_ROWS, c_act);
    ens_add(s_st, ES_FAILED, c_failed);
    ens_add(s_st, ES_FALSE_FAILED, c_ff);
    ens_add(s_st, ES_FALSE_DETECTIONS, c_fd);
    ens_add(s_st, ES_SENT, c_sent);
    ens_add(s_st, ES_DROPPED, c_drop);
    __syncthreads();
    if (tid < n) {
      d.alive[vb + tid] = s_alive[tid];
      d.det_cnt[vb + tid] = s_dcnt[pb * NM + tid];
      d.det_min[vb + tid] = s_dmin[pb * NM + tid];
      d.first[vb + tid] = my_first;
      d.fp[vb + tid] = my_fp;
    }
    if (tid < GH_ENS_NSTAT) {
      long long* st = d.st + b * GH_ENS_NSTAT;
      if (tid == ES_ROUNDS)
        st[tid] += rounds;
      else if (tid == ES_LAST_ROUND)
        st[tid] = (long long)r0 + rounds;
      else
        st[tid] += (long long)s_st[tid];
    }
    if (tid == 0) d.round[b] = r0 + rounds;
  }
}

__global__ __launch_bounds__(256) void k_ens_fill(int32_t* p, int64_t n, int32_t v) {
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (int64_t)gridDim.x * blockDim.x)
    p[x] = v;
}

template <int NM>
hipError_t ens_prepare() {
  // above 64 KiB a kernel's dynamic LDS needs the opt-in (bucket 128)
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ens_step<NM>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)EnsLds<NM>::bytes);
}

template <int NM>
int ens_occupancy() {
  int nb = 0;
  if (ens_prepare<NM>() != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_ens_step<NM>, 8 * NM, EnsLds<NM>::bytes) != hipSuccess) {
    (void)hipGetLastError();
    nb = 1;
  }
  return nb < 1 ? 1 : nb;
}

template <int NM>
hipError_t ens_launch(const GhEns& d, int32_t rounds, int grid, hipStream_t s) {
  const hipError_t rc = ens_prepare<NM>();
  if (rc != hipSuccess) return rc;
  hipLaunchKernelGGL(k_ens_step<NM>, dim3(grid), dim3(8 * NM), EnsLds<NM>::bytes, s, d, rounds);
  return hipGetLastError();
}

}  // namespace

size_t gh_ens_lds_bytes(int bucket) {
  return bucket == 16 ? EnsLds<16>::bytes : bucket == 32 ? EnsLds<32>::bytes : bucket == 64 ? EnsLds<64>::bytes
                                                                                           : EnsLds<128>::bytes;
}

int gh_ens_blocks_per_cu(int bucket) {
  return bucket == 16 ? ens_occupancy<16>() : bucket == 32 ? ens_occupancy<32>() : bucket == 64 ? ens_occupancy<64>()
                                                                                              : ens_occupancy<128>();
}

hipError_t gh_ens_launch(const GhEns& d, int32_t rounds, int grid, hipStream_t s) {
  switch (gh_ens_bucket(d.n)) {
    case 16: return ens_launch<16>(d, rounds, grid, s);
    case 32: return ens_launch<32>(d, rounds, grid, s);
    case 64: return ens_launch<64>(d, rounds, grid, s);
    default: return ens_launch<128>(d, rounds, grid, s);
  }
}

void gh_ens_fill(int32_t* p, int64_t n, int32_t v, hipStream_t s) {
  if (n <= 0) return;
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(k_ens_fill, dim3(grid), dim3(256), 0, s, p, n, v);
}
