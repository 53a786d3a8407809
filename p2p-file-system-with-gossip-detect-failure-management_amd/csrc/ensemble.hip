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
//
// Modes (k_ens_step<NM, RING, QUIRK>; gh_ens_config.peer_mode / detect_mode).
// <NM, false, false> is the kernel above, unchanged: every mode branch is an
// `if constexpr` and EnsLds a function of the modes, so its code, LDS bytes,
// registers and workgroups per CU are what they were.
//
// RING (SPEC §2 step 6 "Ring mode", ID order). No peers are drawn in phase A
// and the pull inboxes s_peer / s_pk do not exist. Phase B ends with each
// row's present mask of the SNAPSHOT (a ballot of the row's lanes: one u64
// word, two at NM = 128) in s_pm, and clears the inbox. Phase C: thread
// (s, q) = (tid / 3, tid % 3), tid < 3 N, of a running active sender s takes
// L and idx by popcounts of s_pm[s], selects target g = the pos-th set bit,
// pos = (idx - 1, idx + 1, idx + 2)[q] mod L (Go's truncated %, + L when
// negative), and when g runs and the message is not lost (block (s, r, q))
// sets bit s of the receiver's INBOX s_inbox[g] (u32 [NM][NM / 32], LDS
// atomicOr); thread (s, 0) counts ring_empty when L = 0. Phase D: a cell takes
// the max of snap[s][c] over the set bits of its row's inbox. A bitmask, not
// the 8 slots of pull mode: with diverged lists one member can be the target
// of every sender. The merge hazard argument holds as above, and for the
// inbox words too: phase D only reads them and writes registers; they are
// cleared in the NEXT round's phase B, behind that round's barrier A, which a
// thread passes only after its phase-D reads, and set again only behind that
// round's barrier B. s_pm is written in phase B and read in phase C of the
// same round, two barriers before its next write.
//
// QUIRK (SPEC §4, ID order). Phase B takes, before anything is tombstoned,
// each cell's candidate flag and the row's present and candidate masks (two
// ballots). A candidate c then decides by bit arithmetic: h = the highest
// present non-candidate bit below c (the list's start when none), o = the
// present bits strictly between h and c (all candidates); detected iff o is
// even or no present bit lies above c (the last entry). At NM <= 64 a row
// lies in one wave: no LDS, no barrier. At NM = 128 a row is two waves: the
// halves meet through s_qm behind one extra barrier (barrier Q, in the
// <128, *, true> instantiations only: five barriers a round, the others
// four), and phase B is split in B1 (guard, heartbeat, flags, masks) and B2
// (detect, clean, snapshot). s_qm is written in B1 and read in B2 of the same
// round; its next write lies behind the next round's barrier A.
//
// No loop here depends on a mask for its trip count: bit selection is six
// halving steps, the inbox walk at most 32 steps per word.
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

template <int NM, bool RING, bool QUIRK>
struct EnsLds {
  static constexpr int PW = NM < 64 ? 1 : NM / 64;  // u64 words of a row's member mask
  static constexpr int IW = NM < 32 ? 1 : NM / 32;  // u32 words of a receiver's inbox
  static constexpr size_t st = 0;                                      // u64 [GH_ENS_NSTAT]
  static constexpr size_t snap = st + 8 * 16;                          // i32 [NM + 1][NM]
  static constexpr size_t cnt = snap + sizeof(int32_t) * (NM + 1) * NM;  // i32 [NM]
  static constexpr size_t dcnt = cnt + 4 * NM;                         // i32 [2][NM]
  static constexpr size_t dmin = dcnt + 8 * NM;                        // i32 [2][NM]
  static constexpr size_t out = dmin + 8 * NM;                         // u32 [NM]
  static constexpr size_t in = out + 4 * NM;                           // u32 [NM]
  static constexpr size_t pk = in + 4 * NM;                            // pull: u8 [NM][8] arrived senders (NM: none)
  static constexpr size_t peer = pk + (RING ? 0 : 8 * NM);             // pull: u8 [NM][8] drawn peers
  static constexpr size_t alive = peer + (RING ? 0 : 8 * NM);          // u8 [NM]
  static constexpr size_t active = alive + NM;                         // u8 [NM]
  static constexpr size_t pm = active + NM;                            // ring: u64 [NM][PW] the snapshot rows' present masks
  static constexpr size_t inbox = pm + (RING ? 8 * NM * PW : 0);       // ring: u32 [NM][IW] arrived senders
  static constexpr size_t qm = inbox + (RING ? 4 * NM * IW : 0);       // quirk, NM = 128: u64 [NM][2][2] (half; present, candidate)
  static constexpr size_t bytes = qm + (QUIRK && NM == 128 ? 32 * NM : 0);
  static_assert(pm % 8 == 0, "the u64 masks are aligned");
};

__device__ __forceinline__ void ens_add(unsigned long long* st, int f, uint32_t v) {
  if (v) atomicAdd(st + f, (unsigned long long)v);
}

// Quirk detection (SPEC §4) of candidate c in a row whose ID-ordered list has
// the present mask (p0, p1) and the candidate mask (c0, c1), bit c of word
// c / 64: detected iff the present entries between c and the nearest present
// non-candidate below it are an even number, or c is the list's last entry.
__device__ __forceinline__ bool ens_quirk_detects(unsigned long long p0, unsigned long long p1, unsigned long long c0,
                                                  unsigned long long c1, int c) {
  // the bits strictly below c (2 << 63 wraps to 0: no shift by 64 anywhere)
  const unsigned long long b0 = c >= 64 ? ~0ull : (1ull << c) - 1ull;
  const unsigned long long b1 = c >= 64 ? (1ull << (c - 64)) - 1ull : 0ull;
  const unsigned long long n0 = p0 & ~c0 & b0, n1 = p1 & ~c1 & b1;
  unsigned long long m0 = b0, m1 = b1;  // strictly between that entry and c
  if (n1) {
    m0 = 0;
    m1 = b1 & ~((2ull << (63 - __clzll((long long)n1))) - 1ull);
  } else if (n0) {
    m0 = b0 & ~((2ull << (63 - __clzll((long long)n0))) - 1ull);
  }
  const int o = __popcll(p0 & m0) + __popcll(p1 & m1);
  const unsigned long long a0 = c >= 64 ? 0ull : ~((2ull << c) - 1ull);  // the bits above c
  const unsigned long long a1 = c >= 64 ? ~((2ull << (c - 64)) - 1ull) : ~0ull;
  return !(o & 1) || !((p0 & a0) | (p1 & a1));
}

// The position of the pos-th set bit of m (0 <= pos < popcount(m)): six halving steps.
__device__ __forceinline__ int ens_select_bit(unsigned long long m, int pos) {
  int base = 0;
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    const unsigned long long low = m & ((1ull << w) - 1ull);
    const int below = __popcll(low);
    if (pos >= below) {
      pos -= below;
      m >>= w;
      base += w;
    } else {
      m = low;
    }
  }
  return base;
}

template <int NM, bool RING, bool QUIRK>
__global__ __launch_bounds__(8 * NM) void k_ens_step(GhEns d, int32_t rounds) {
  constexpr int CPT = NM / 8;  // rows (cells) per thread
  constexpr int RW = NM < 64 ? NM : 64;  // lanes of a wave in one row
  using L = EnsLds<NM, RING, QUIRK>;
  constexpr int PW = L::PW, IW = L::IW;
  extern __shared__ __align__(16) unsigned char lds[];
  unsigned long long* s_st = reinterpret_cast<unsigned long long*>(lds + L::st);
  int32_t* s_snap = reinterpret_cast<int32_t*>(lds + L::snap);
  int32_t* s_cnt = reinterpret_cast<int32_t*>(lds + L::cnt);
  int32_t* s_dcnt = reinterpret_cast<int32_t*>(lds + L::dcnt);
  int32_t* s_dmin = reinterpret_cast<int32_t*>(lds + L::dmin);
  uint32_t* s_out = reinterpret_cast<uint32_t*>(lds + L::out);
  uint32_t* s_in = reinterpret_cast<uint32_t*>(lds + L::in);
  [[maybe_unused]] uint8_t* s_pk = lds + L::pk;
  [[maybe_unused]] uint8_t* s_peer = lds + L::peer;
  uint8_t* s_alive = lds + L::alive;
  uint8_t* s_active = lds + L::active;
  [[maybe_unused]] unsigned long long* s_pm = reinterpret_cast<unsigned long long*>(lds + L::pm);
  [[maybe_unused]] uint32_t* s_inbox = reinterpret_cast<uint32_t*>(lds + L::inbox);
  [[maybe_unused]] unsigned long long* s_qm = reinterpret_cast<unsigned long long*>(lds + L::qm);

  const int tid = threadIdx.x;
  const int n = d.n, k = d.k;
  const int c = tid % NM, ro = tid / NM;  // this thread's column, and its row within each group of 8
  const int lane = tid & 63;
  // the lanes of this thread's row in its wave
  const unsigned long long rowmask = RW == 64 ? ~0ull : ((1ull << RW) - 1ull) << ((lane / RW) * RW);
  [[maybe_unused]] const int rsh = RW == 64 ? 0 : (lane / RW) * RW;  // the row's first lane in its wave
  [[maybe_unused]] const int li = tid >> 3, lt = tid & 7;  // phase C, pull: receiver and draw
  [[maybe_unused]] const int rs = tid / 3, rq = tid - 3 * rs;  // phase C, ring: sender and slot

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
    [[maybe_unused]] const bool li_runs = lt < k && li < n && s_alive[li];
    const bool me_runs = tid < n && s_alive[tid];

    uint32_t c_tomb = 0, c_unk = 0, c_det = 0, c_rel = 0, c_mrg = 0, c_act = 0;
    uint32_t c_failed = 0, c_ff = 0, c_fd = 0, c_sent = 0, c_drop = 0;
    [[maybe_unused]] uint32_t c_empty = 0;
    int pb = 0;  // the REMOVE set pending this round

    for (int32_t q = 0; q < rounds; ++q) {
      const int32_t r = r0 + 1 + q;
      // r >= 1 and T >= 0: r - T fits an int32
      const int32_t r_fail = r - par.t_fail, r_clean = r - par.t_cleanup;
      // ---- phase A: peers; REMOVE delivery (step 1); row counts ---------------
      if (!RING && me_runs) {
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
      if constexpr (RING) {
        if (tid < NM * IW) s_inbox[tid] = 0;  // (last round's phase D is done with it: barrier A)
      }
      [[maybe_unused]] uint32_t cbits = 0;  // quirk, NM = 128: bit j = the cell of row 8 j + ro is a candidate
      if constexpr (QUIRK && NM == 128) {
        // B1: steps 2-3 and the candidates; the row's two half masks meet in LDS
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
          if (8 * j >= n) continue;  // (uniform: rows outside N)
          const int i = 8 * j + ro;
          const bool run = (amask >> j) & 1u;
          const bool act = run && s_cnt[i] >= d.min_members;
          if (run && !act) {
            if (hb[j] >= 0) ts[j] = r;
          } else if (act && c == i && hb[j] >= 0) {
            ++hb[j];
            ts[j] = r;
          }
          const bool cd = act && c != i && hb[j] > 1 && ts[j] < r_fail;
          const unsigned long long pmk = __ballot(hb[j] >= 0), cmk = __ballot(cd);
          if (lane == 0) {
            s_qm[4 * i + 2 * (c >> 6)] = pmk;
            s_qm[4 * i + 2 * (c >> 6) + 1] = cmk;
          }
          cbits |= (uint32_t)cd << j;
        }
        __syncthreads();  // barrier Q
      }
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        if (8 * j >= n) continue;  // (uniform: rows outside N)
        const int i = 8 * j + ro;
        const bool run = (amask >> j) & 1u;
        const bool act = run && s_cnt[i] >= d.min_members;
        if constexpr (!QUIRK) {
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
        } else {
          bool cd;
          unsigned long long p0, p1 = 0, c0, c1 = 0;
          if constexpr (NM == 128) {
            cd = (cbits >> j) & 1u;
            p0 = s_qm[4 * i];  // (one address per wave: a broadcast)
            c0 = s_qm[4 * i + 1];
            p1 = s_qm[4 * i + 2];
            c1 = s_qm[4 * i + 3];
          } else {
            if (run && !act) {
              if (hb[j] >= 0) ts[j] = r;  // the <4 guard: the row only stamps its list
            } else if (act && c == i && hb[j] >= 0) {
              ++hb[j];
              ts[j] = r;
            }
            cd = act && c != i && hb[j] > 1 && ts[j] < r_fail;
            // the row's list and its candidates, before anything is tombstoned
            p0 = (__ballot(hb[j] >= 0) & rowmask) >> rsh;
            c0 = (__ballot(cd) & rowmask) >> rsh;
          }
          if (cd && ens_quirk_detects(p0, p1, c0, c1, c)) {
            hb[j] = GH_TOMBSTONE;
            ++c_det;
            atomicAdd(&s_dcnt[(pb ^ 1) * NM + c], 1);
            atomicMin(&s_dmin[(pb ^ 1) * NM + c], i);
          }
          if (act && hb[j] == GH_TOMBSTONE && ts[j] < r_clean) {
            hb[j] = GH_ABSENT;
            ++c_rel;
          }
        }
        s_snap[8 * NM * j + tid] = hb[j];  // (= [i][c]: tid = ro * NM + c)
        if constexpr (RING) {
          const unsigned long long sp = __ballot(hb[j] >= 0);
          if ((lane & (RW - 1)) == 0) s_pm[PW * i + (NM == 128 ? c >> 6 : 0)] = (sp & rowmask) >> rsh;
        }
        if (c == 0) {
          s_active[i] = act;
          c_act += act;
        }
      }
      __syncthreads();
      // ---- phase C: which draws arrive (step 6a); the round's record ----------
      if constexpr (RING) {
        // thread (rs, rq): slot rq of sender rs (ring form of steps 6 and 6a)
        if (tid < 3 * n && s_alive[rs] && s_active[rs]) {
          const unsigned long long p0 = s_pm[PW * rs], p1 = PW > 1 ? s_pm[PW * rs + PW - 1] : 0ull;
          const int n0 = __popcll(p0), len = n0 + __popcll(p1);
          if (len == 0) {
            c_empty += rq == 0;  // (the reference divides by zero here: D3)
          } else {
            const unsigned long long w = rs >= 64 ? p1 : p0, bit = 1ull << (rs & 63);
            const int idx = (w & bit) ? (rs >= 64 ? n0 : 0) + __popcll(w & (bit - 1ull)) : -1;
            int pos = (idx + (rq == 0 ? -1 : rq)) % len;  // truncated, as Go's
            if (pos < 0) pos += len;
            const int g = pos < n0 ? ens_select_bit(p0, pos) : 64 + ens_select_bit(p1, pos - n0);
            if (s_alive[g]) {
              ++c_sent;
              bool lost = false;
              if (lossy) {
                uint32_t w4[4];
                gh_philox_block(par.seed, (uint32_t)rs, (uint32_t)r, GH_TAG_LINK, (uint32_t)rq, w4);
                lost = gh_link_hit(s_out[rs], w4[0]) || gh_link_hit(s_in[g], w4[1]);
              }
              if (lost)
                ++c_drop;
              else
                atomicOr(&s_inbox[IW * g + (rs >> 5)], 1u << (rs & 31));
            }
          }
        }
      } else {
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
        int32_t m = GH_ABSENT;
        if constexpr (RING) {
          // the row's inbox: one address per row, so wave-uniform at NM >= 64
#pragma unroll
          for (int w = 0; w < IW; ++w) {
            uint32_t bits = s_inbox[IW * (8 * j + ro) + w];
            for (int t = 0; t < 32 && bits; ++t) {
              m = max(m, s_snap[(32 * w + __ffs((int)bits) - 1) * NM + c]);
              bits &= bits - 1u;
            }
          }
        } else {
          const unsigned long long snd = reinterpret_cast<const unsigned long long*>(s_pk)[8 * j + ro];
          for (int t = 0; t < k; ++t) m = max(m, s_snap[(int)((snd >> (8 * t)) & 0xFFu) * NM + c]);
        }
        if (hb[j] >= GH_ABSENT && m > hb[j]) {
          hb[j] = m;
          ts[j] = r;
          ++c_mrg;
        }
      }
      pb ^= 1;
      // (no barrier: the next round writes s_peer and s_cnt, which phase D does
      // not read, and reaches the snapshot, s_pk and the ring inbox only behind
      // its barrier A)
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
    if constexpr (RING) ens_add(s_st, ES_RING_EMPTY, c_empty);
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

template <int NM, bool RING, bool QUIRK>
hipError_t ens_prepare() {
  // above 64 KiB a kernel's dynamic LDS needs the opt-in (bucket 128)
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ens_step<NM, RING, QUIRK>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)EnsLds<NM, RING, QUIRK>::bytes);
}

template <int NM, bool RING, bool QUIRK>
int ens_occupancy() {
  int nb = 0;
  if (ens_prepare<NM, RING, QUIRK>() != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_ens_step<NM, RING, QUIRK>, 8 * NM,
                                                   EnsLds<NM, RING, QUIRK>::bytes) != hipSuccess) {
    (void)hipGetLastError();
    nb = 1;
  }
  return nb < 1 ? 1 : nb;
}

template <int NM, bool RING, bool QUIRK>
hipError_t ens_launch(const GhEns& d, int32_t rounds, int grid, hipStream_t s) {
  const hipError_t rc = ens_prepare<NM, RING, QUIRK>();
  if (rc != hipSuccess) return rc;
  constexpr size_t lds_bytes = EnsLds<NM, RING, QUIRK>::bytes;
  hipLaunchKernelGGL((k_ens_step<NM, RING, QUIRK>), dim3(grid), dim3(8 * NM), lds_bytes, s, d, rounds);
  return hipGetLastError();
}

// The instantiation of (bucket, ring, quirk) as a tag f is called with.
template <int NM, bool RING, bool QUIRK>
struct EnsInst {
  static constexpr int nm = NM;
  static constexpr bool ring = RING, quirk = QUIRK;
};

template <int NM, class F>
auto ens_pick_modes(bool ring, bool quirk, F&& f) {
  if (ring) return quirk ? f(EnsInst<NM, true, true>{}) : f(EnsInst<NM, true, false>{});
  return quirk ? f(EnsInst<NM, false, true>{}) : f(EnsInst<NM, false, false>{});
}

template <class F>
auto ens_pick(int bucket, bool ring, bool quirk, F&& f) {
  switch (bucket) {
    case 16: return ens_pick_modes<16>(ring, quirk, f);
    case 32: return ens_pick_modes<32>(ring, quirk, f);
    case 64: return ens_pick_modes<64>(ring, quirk, f);
    default: return ens_pick_modes<128>(ring, quirk, f);
  }
}

}  // namespace

size_t gh_ens_lds_bytes(int bucket, bool ring, bool quirk) {
  return ens_pick(bucket, ring, quirk, [](auto t) -> size_t {
    using T = decltype(t);
    return EnsLds<T::nm, T::ring, T::quirk>::bytes;
  });
}

int gh_ens_blocks_per_cu(int bucket, bool ring, bool quirk) {
  return ens_pick(bucket, ring, quirk, [](auto t) -> int {
    using T = decltype(t);
    return ens_occupancy<T::nm, T::ring, T::quirk>();
  });
}

hipError_t gh_ens_launch(const GhEns& d, int32_t rounds, int grid, hipStream_t s) {
  return ens_pick(gh_ens_bucket(d.n), d.ring != 0, d.quirk != 0, [&](auto t) -> hipError_t {
    using T = decltype(t);
    return ens_launch<T::nm, T::ring, T::quirk>(d, rounds, grid, s);
  });
}

void gh_ens_fill(int32_t* p, int64_t n, int32_t v, hipStream_t s) {
  if (n <= 0) return;
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(k_ens_fill, dim3(grid), dim3(256), 0, s, p, n, v);
}
