// Membership groups and view digests (gh_groups; DESIGN.md "Groups"): the
// weakly connected components of "running i lists running c" over the
// current buffer, labelled by their lowest member id, and per running row a
// 64-bit digest of the set of members it lists. Read-only. No reference
// counterpart (the nearest is comparing the `lsm` of every VM by hand,
// slave/slave.go:558-561).
//
// Labels are member ids that only decrease. One PASS is
//   k_groups   the table walk, census.hip's grid: (tile, row block), 256
//              threads, a lane owns one 8-column chunk column of the tile and
//              walks the block's rows; stopped rows are skipped before any
//              table read (the block's row labels are staged in LDS, a stopped
//              row's is "none"). The lane keeps the labels of its 8 columns
//              in registers for the whole walk. Per running row i it takes the
//              lowest label among the row's listed running columns (lane-local,
//              then a shuffle reduce over the lanes of the row's segment, then
//              one global atomic per (row, block), only where it improves on
//              the row's label), and per column the lowest label of the rows
//              listing it (registers, then LDS, then one global atomic per
//              (column, block) that improves). The first pass also adds
//              mix(c) of every listed cell into the row's digest: a lane sum,
//              the same reduce, one 64-bit atomic add per (row, block).
//              A wave whose lanes all see full rows (the healthy cluster) skips
//              the reduces: its rows take the tile's constants.
//              No per-edge atomics; everything is integer min / sum, so tiles,
//              blocks and shards combine in any order and the result is exact.
//   k_hook_m   O(N): m[v] = min(label[v], rowmin[v], colmin[v]), old[v] =
//              label[v]; sets `changed` where m[v] < label[v]
//   k_hook     O(N): atomicMin(label[old[v]], m[v]) (the root takes the hook)
//              and atomicMin(label[v], m[v]); reads only k_hook_m's outputs, so
//              the labels after it do not depend on the thread order and every
//              shard computes the same ones
//   k_jump     O(N): every label to its root (labels are roots or point to a
//              lower id of the same component: a forest)
// and the host repeats passes until `changed` stays 0. Minima are kept as
// maxima of INT32_MAX - x (0 = none), the form the shards' MAX-only transport
// reduces, as census.hip's cmin.
#include <algorithm>

#include "gh_internal.h"

namespace {

constexpr int kColMax = 256;    // widest tile
constexpr int kRowsMax = 4096;  // rows per block at most (their labels in LDS: 16 KiB)
#ifndef GH_GROUPS_WGS
#define GH_GROUPS_WGS 8192      // workgroups a launch aims for (census.hip's choice)
#endif

__device__ __forceinline__ unsigned long long groups_mix(unsigned long long c) {
  unsigned long long z = (c + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Listed cells (bit j = cell j) of a chunk of 16-bit codes that is no marker:
// offset 1023 is absent or a tombstone; flagged cells are listed.
__device__ __forceinline__ uint32_t listed16(const uint4& x) {
  const uint32_t w[4] = {x.x, x.y, x.z, x.w};
  uint32_t pm = 0u;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const uint32_t off = pk_lshr16(w[m], 5) & 0x03FF03FFu;
    const uint32_t ls = ~pk_zero_mask(off ^ 0x03FF03FFu);
    pm |= (ls & 1u) << (2 * m) | ((ls >> 16) & 1u) << (2 * m + 1);
  }
  return pm;
}
// ... of a tier chunk's lag word: every nibble other than 15 (the row's own
// cell carries the diagonal's code, 1..12: listed)
__device__ __forceinline__ uint32_t listed4(uint32_t u) {
  uint32_t n15 = u & (u >> 1);
  n15 &= (n15 >> 2);
  const uint32_t p = ~n15 & 0x11111111u;
  uint32_t pm = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) pm |= ((p >> gh_nib(j)) & 1u) << j;
  return pm;
}
// ... of the 16-bit chunk x of row i, local column c: wide and frozen markers
// through the decoder
__device__ __forceinline__ uint32_t listed_chunk(const GhDev& d, int cur, int64_t i, int64_t c, int32_t r,
                                                 const uint4& x) {
  const uint32_t h0 = x.x & 0xFFFFu;
  if (h0 != GH_N_WIDE && h0 != GH_N_FROZEN) return listed16(x);
  GhCell v[8];
  gh_dec8(d, cur, i, c, r, x, v);
  uint32_t pm = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) pm |= (v[j].x >= 0 ? 1u : 0u) << j;
  return pm;
}

template <bool TIER, bool FIRST>
__device__ __forceinline__ void groups_block(const GhDev& d, int cur, int32_t r, int64_t rpb, const GhGroups& o,
                                             int32_t* lds) {
  const int tid = threadIdx.x;
  const int lgc = d.lgtw - 3;            // log2(chunks per segment)
  const int gl = 1 << lgc;               // lanes per (tile, row) segment, <= 32
  const int q = tid & (gl - 1);          // the lane's chunk column in the tile
  const int64_t rsub = tid >> lgc, rstep = 256 >> lgc;
  const int64_t tile = blockIdx.x;
  const int64_t c = tile * d.tw + q * 8; // local column of the lane's chunks
  const int64_t s0 = (int64_t)blockIdx.y * rpb, s1 = min<int64_t>(s0 + rpb, d.nrows);
  if (tile * d.tw >= d.ncol) return;     // a tile of padding only

  int32_t* rl = lds;                     // [rpb] INT32_MAX - label of the block's rows, 0 = stopped
  int32_t* cl = lds + kRowsMax;          // [tw] the block's column maxima
  for (int64_t x = tid; x < s1 - s0; x += 256) {
    const int32_t l = o.label[d.row0 + s0 + x];
    rl[x] = l < 0 ? 0 : INT32_MAX - l;
  }
  cl[tid] = 0;

  // the lane's columns: valid ones (not padding), their labels (0: a stopped
  // member or padding, no edge) and mix values
  uint32_t vm = 0u;
  int32_t lab[8], cm[8];
  unsigned long long mx[8];
  int32_t lmax = 0;
  unsigned long long ltot = 0ull;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    lab[j] = cm[j] = 0;
    mx[j] = 0ull;
    if (c + j < d.ncol) {
      vm |= 1u << j;
      const int32_t l = o.label[d.col0 + c + j];
      lab[j] = l < 0 ? 0 : INT32_MAX - l;
      if (FIRST) mx[j] = groups_mix((unsigned long long)(d.col0 + c + j));
    }
    lmax = max(lmax, lab[j]);
    ltot += mx[j];
  }
  // what a full row takes from the whole tile (every segment's lanes cover it)
  int32_t tmax = lmax;
  unsigned long long ttot = ltot;
  for (int w = 1; w < gl; w <<= 1) {
    tmax = max(tmax, __shfl_xor(tmax, w));
    if (FIRST) ttot += __shfl_xor(ttot, w);
  }
  __syncthreads();

  const int64_t tcell = tile * d.tstride + q * 8;
  constexpr int UN = 4;  // rows in flight per lane
  for (int64_t sb = s0 + rsub; sb < s1; sb += UN * rstep) {
    int32_t rlc[UN];
    uint32_t aw[UN], uw[UN];
    uint4 xs[UN];
#pragma unroll
    for (int k = 0; k < UN; ++k) {
      const int64_t s = sb + k * rstep;
      rlc[k] = s < s1 ? rl[s - s0] : 0;  // 0: a stopped row has no edges and no digest
      aw[k] = uw[k] = 0u;
      xs[k] = uint4{0u, 0u, 0u, 0u};
      if (!rlc[k] || !vm) continue;
      const int64_t cell = tcell + (s << d.lgtw);
      if (TIER) {
        aw[k] = d.a4[cur][cell >> 3];
        uw[k] = d.pl[cur][cell >> 3];
      } else {
        xs[k] = *reinterpret_cast<const uint4*>(d.hn[cur] + cell);
      }
    }
    uint32_t pm[UN];
    bool full = true;
#pragma unroll
    for (int k = 0; k < UN; ++k) {
      pm[k] = 0u;
      if (!rlc[k] || !vm) continue;
      const int64_t s = sb + k * rstep, i = d.row0 + s;
      if (TIER && !gh_t4_esc(aw[k])) {
        pm[k] = listed4(uw[k]) & vm;
      } else {
        if (TIER) xs[k] = *reinterpret_cast<const uint4*>(d.hn[cur] + tcell + (s << d.lgtw));  // an escaped chunk
        pm[k] = listed_chunk(d, cur, i, c, r, xs[k]) & vm;
      }
      full = full && pm[k] == vm;
    }
    if (__all(full)) {
      // every lane of the wave lists all of its columns in all of its rows
#pragma unroll
      for (int k = 0; k < UN; ++k) {
        if (!rlc[k]) continue;
#pragma unroll
        for (int j = 0; j < 8; ++j) cm[j] = max(cm[j], rlc[k]);
        if (q == 0) {
          const int64_t i = d.row0 + sb + k * rstep;
          if (tmax > rlc[k]) atomicMax(&o.rmax[i], tmax);
          if (FIRST) atomicAdd(&o.digest[i], ttot);
        }
      }
      continue;
    }
#pragma unroll
    for (int k = 0; k < UN; ++k) {
      if (!rlc[k]) continue;  // (the same for every lane of the segment)
      int32_t rm = 0;
      unsigned long long ds = 0ull;
      if (pm[k] == vm) {
        rm = lmax;
        ds = ltot;
#pragma unroll
        for (int j = 0; j < 8; ++j) cm[j] = max(cm[j], rlc[k]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool p = ((pm[k] >> j) & 1u) != 0;
          rm = max(rm, p ? lab[j] : 0);
          cm[j] = max(cm[j], p ? rlc[k] : 0);
          if (FIRST) ds += p ? mx[j] : 0ull;
        }
      }
      for (int w = 1; w < gl; w <<= 1) {
        rm = max(rm, __shfl_xor(rm, w));
        if (FIRST) ds += __shfl_xor(ds, w);
      }
      if (q == 0) {
        const int64_t i = d.row0 + sb + k * rstep;
        if (rm > rlc[k]) atomicMax(&o.rmax[i], rm);
        if (FIRST && ds) atomicAdd(&o.digest[i], ds);
      }
    }
  }
  // the lanes' columns into the block's, the block's into the shard's
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (cm[j] > lab[j] && lab[j]) atomicMax(&cl[q * 8 + j], cm[j]);
  __syncthreads();
  const int64_t cg = tile * d.tw + tid;
  if (tid < d.tw && cg < d.ncol && cl[tid]) atomicMax(&o.cmax[d.col0 + cg], cl[tid]);
}

// Which of the two forms runs is the buffer's own flag (m8, device side):
// both are launched and the other returns at once, as k_census does.
template <bool TIER, bool FIRST>
__global__ __launch_bounds__(256, 4) void k_groups(GhDev d, int cur, int32_t r, int64_t rpb, GhGroups o) {
  __shared__ int32_t lds[kRowsMax + kColMax];
  if (gh_m8(d, cur) != TIER) return;
  groups_block<TIER, FIRST>(d, cur, r, rpb, o, lds);
}

// label[v] = v for a running member, -1 for a stopped one
__global__ void k_groups_init(GhGroups o, const uint8_t* alive, int32_t n) {
  const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) o.label[v] = alive[v] ? v : -1;
}

__global__ void k_hook_m(GhGroups o, int32_t n) {
  const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int32_t l = o.label[v];
  int32_t m = l;
  if (l >= 0) {
    const int32_t x = max(o.rmax[v], o.cmax[v]);
    if (x > 0) m = min(l, INT32_MAX - x);
    if (m < l) o.flag[0] = 1;
  }
  o.rmax[v] = m;  // (both are cleared by k_hook for the next pass)
  o.cmax[v] = l;
}

__global__ void k_hook(GhGroups o, int32_t n) {
  const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int32_t m = o.rmax[v], l = o.cmax[v];
  o.rmax[v] = o.cmax[v] = 0;
  if (l >= 0 && m < l) {
    atomicMin(&o.label[l], m);
    atomicMin(&o.label[v], m);
  }
}

__global__ void k_jump(GhGroups o, int32_t n) {
  const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  int32_t l = o.label[v];
  if (l < 0) return;
  // concurrent writes only replace a label by one further down its own chain
  for (int32_t p = o.label[l]; p != l; p = o.label[l]) l = p;
  o.label[v] = l;
}

}  // namespace

void launch_groups_init(const GhDev& d, const GhGroups& o, hipStream_t s) {
  hipLaunchKernelGGL(k_groups_init, dim3((d.n + 255) / 256), dim3(256), 0, s, o, d.alive, d.n);
}

void launch_groups_walk(const GhDev& d, int cur, int32_t r, const GhGroups& o, int first, hipStream_t s) {
  if (d.nrows <= 0 || d.ncol <= 0) return;
  // census.hip's row blocks: enough workgroups to fill the device, at least
  // 64 rows each, at most kRowsMax (the block's row labels sit in LDS)
  const int64_t rstep = 256 / (d.tw / 8);
  const int64_t want = std::max<int64_t>(1, GH_GROUPS_WGS / d.ntiles);
  int64_t rpb = std::max<int64_t>(64, (d.nrows + want - 1) / want);
  rpb = std::min<int64_t>((rpb + rstep - 1) / rstep * rstep, kRowsMax);
  const int64_t nrb = (d.nrows + rpb - 1) / rpb;
  const dim3 grid((unsigned)d.ntiles, (unsigned)nrb);
  if (first) {
    if (d.a4[0]) hipLaunchKernelGGL((k_groups<true, true>), grid, dim3(256), 0, s, d, cur, r, rpb, o);
    hipLaunchKernelGGL((k_groups<false, true>), grid, dim3(256), 0, s, d, cur, r, rpb, o);
  } else {
    if (d.a4[0]) hipLaunchKernelGGL((k_groups<true, false>), grid, dim3(256), 0, s, d, cur, r, rpb, o);
    hipLaunchKernelGGL((k_groups<false, false>), grid, dim3(256), 0, s, d, cur, r, rpb, o);
  }
}

void launch_groups_hook_m(const GhDev& d, const GhGroups& o, hipStream_t s) {
  hipLaunchKernelGGL(k_hook_m, dim3((d.n + 255) / 256), dim3(256), 0, s, o, d.n);
}

void launch_groups_hook(const GhDev& d, const GhGroups& o, hipStream_t s) {
  hipLaunchKernelGGL(k_hook, dim3((d.n + 255) / 256), dim3(256), 0, s, o, d.n);
  hipLaunchKernelGGL(k_jump, dim3((d.n + 255) / 256), dim3(256), 0, s, o, d.n);
}
