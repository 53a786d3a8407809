// Cluster ensembles (gh_ens_*, SPEC §11; DESIGN.md "Ensemble"): the device
// state of B independent clusters of N <= GH_ENS_MAX_MEMBERS members and the
// launchers of ensemble.hip. Nothing here is shared with an ordinary engine
// (GhDev): an ensemble has its own handle, buffers and stream.
//
// HBM layout, cluster b: exact int32 tables hb / ts [b][N][N] (row-major, no
// padding; GH_ABSENT / GH_TOMBSTONE as in SPEC §1, ts kept for every cell),
// alive / crashq [b][N] (crashq: the GH_EV_CRASH events queued for the next
// round run), the pending REMOVE set det_cnt / det_min [b][N] (D_{r-1}: the
// rows that detected member c in the last round and the lowest of them, N
// when none), round [b], the loss thresholds out / in [b][N], the detect
// record first / fp [b][N] and the statistics of the current gh_ens_step call
// st [b][GH_ENS_NSTAT] (gh_ens_stats as 14 int64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gossiphip.h"

#define GH_ENS_NSTAT 14             // int64 fields of gh_ens_stats
#define GH_ENS_LAUNCH_ROUNDS (1 << 20)  // rounds per launch at most: a thread's 32-bit counters hold them

struct GhEns {
  int32_t n, k, min_members;
  uint8_t ring, quirk;  // GH_PEER_RING / GH_DETECT_QUIRK: which k_ens_step runs (the layout's padding: nothing moves)
  int64_t nb;  // clusters B
  int32_t *hb, *ts;
  uint8_t *alive, *crashq;
  int32_t *det_cnt, *det_min;
  int32_t* round;
  const gh_ens_params* par;
  const uint32_t *out, *in;
  int32_t *first, *fp;
  long long* st;
};

// Size bucket (the kernel's row stride in LDS) of N members: 16, 32, 64, 128.
inline int gh_ens_bucket(int n) { return n <= 16 ? 16 : n <= 32 ? 32 : n <= 64 ? 64 : 128; }
// The kernel is instantiated per (bucket, ring, quirk); the three calls below
// dispatch on all three.
// LDS bytes of one workgroup of that instantiation.
size_t gh_ens_lds_bytes(int bucket, bool ring, bool quirk);
// Workgroups of that instantiation one CU holds (the occupancy query; >= 1).
int gh_ens_blocks_per_cu(int bucket, bool ring, bool quirk);
// Runs `rounds` (1..GH_ENS_LAUNCH_ROUNDS) rounds of every cluster on `grid`
// workgroups in the modes d carries, adding the statistics to d.st.
hipError_t gh_ens_launch(const GhEns& d, int32_t rounds, int grid, hipStream_t s);
// Fills p[0, n) with v.
void gh_ens_fill(int32_t* p, int64_t n, int32_t v, hipStream_t s);
