// Membership census (gh_census; DESIGN.md "Census"): per member column, how
// the running rows see it -- observers listing it, observers holding it
// tombstoned, min / max / sum of the listed heartbeats, the oldest entry --
// and the age histogram of every listed cell, in one read-only pass over the
// current buffer. No reference counterpart (the nearest is `lsm`,
// slave/slave.go:558-561, on every VM).
//
//   k_census   grid (tile, row block), 256 threads. A lane owns one 8-column
//              chunk column of the tile and walks the block's rows, so a wave
//              reads whole (tile, row) segments side by side: with 256-member
//              tiles two rows per step, 128 B of lag nibbles and 128 B of age
//              nibbles each. Stopped rows are skipped before any table read.
//              A chunk is accumulated on its codes, in the column's frame
//              (the tier's lag nibbles, or the 16-bit codes' offsets), in
//              packed 16-bit halves, one pair of cells per register, and
//              converted to heartbeats once per lane. A chunk that has no
//              such codes -- an escaped chunk of a tier buffer, a wide or
//              frozen marker of a 16-bit one -- is decoded (gh_dec8) straight
//              into the block's accumulators. A wave counts ages in its own
//              LDS bins, one column per lane (no bank conflict, no contention).
//              The lanes of a block meet in LDS, the blocks of a column in
//              global atomics; everything is integer, so the order is free.
#include <algorithm>

#include "gh_internal.h"

namespace {

constexpr int kBins = GH_CENSUS_BINS;
constexpr int kHistWords = 4 * kBins * 64;  // per wave [bin][lane]
constexpr int kColMax = 256;                // widest tile
constexpr int kRowsMax = 4096;              // rows per block at most (16 per thread)
#ifndef GH_CENSUS_WGS
#define GH_CENSUS_WGS 8192                  // workgroups a launch aims for (A/B: DESIGN.md "Census")
#endif

__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
  return as_u(__builtin_elementwise_max(as_us(a), as_us(b)));
}

// The block's per-column accumulators (LDS), in the form the shards reduce.
struct ColAcc {
  int32_t *listed, *tomb, *cmin, *hmax, *amax;
  unsigned long long* sum;
  __device__ __forceinline__ void add(int cc, int32_t n, int32_t lo, int32_t hi, unsigned long long s,
                                      int32_t age) const {
    atomicAdd(&listed[cc], n);
    atomicMax(&cmin[cc], INT32_MAX - lo);
    atomicMax(&hmax[cc], hi);
    atomicMax(&amax[cc], age);
    atomicAdd(&sum[cc], s);
  }
};

// A decoded chunk (row i, local columns c..c+7) straight into the block's
// accumulators and bins bh: the chunks the walk cannot take on their codes.
__device__ __forceinline__ void census_cells(const GhDev& d, int64_t i, int64_t c, int32_t r, const GhCell v[8],
                                             unsigned long long* bh, const ColAcc& ca, int cc0) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (c + j >= d.ncol || d.col0 + c + j == i) continue;  // padding; the row's own entry
    const int32_t x = v[j].x;
    if (x >= 0) {
      const int64_t a64 = (int64_t)r - v[j].ts;
      const int32_t a = a64 < 0 ? 0 : a64 > INT32_MAX ? INT32_MAX : (int32_t)a64;
      atomicAdd(&bh[a < kBins - 1 ? a : kBins - 1], 1ull);
      ca.add(cc0 + j, 1, x, x, (unsigned long long)x, a);
    } else if (x == GH_TOMBSTONE) {
      atomicAdd(&ca.tomb[cc0 + j], 1);
    }
  }
}

template <bool TIER>
__device__ __forceinline__ void census_block(const GhDev& d, int cur, int32_t r, int64_t rpb, const GhCensus& o,
                                             uint32_t* lds) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lgc = d.lgtw - 3;                // log2(chunks per segment)
  const int q = tid & ((1 << lgc) - 1);      // the lane's chunk column in the tile
  const int64_t rsub = tid >> lgc, rstep = 256 >> lgc;
  const int64_t tile = blockIdx.x;
  const int64_t c = tile * d.tw + q * 8;     // local column of the lane's chunks
  const int cc0 = q * 8;
  const int64_t s0 = (int64_t)blockIdx.y * rpb, s1 = min<int64_t>(s0 + rpb, d.nrows);

  uint32_t* hw = lds + wave * (kBins * 64) + lane;
  ColAcc ca;
  ca.listed = reinterpret_cast<int32_t*>(lds + kHistWords);
  ca.tomb = ca.listed + kColMax;
  ca.cmin = ca.tomb + kColMax;
  ca.hmax = ca.cmin + kColMax;
  ca.amax = ca.hmax + kColMax;
  ca.sum = reinterpret_cast<unsigned long long*>(ca.amax + kColMax);
  unsigned long long* bh = ca.sum + kColMax;  // the block's bins
  for (int x = tid; x < kHistWords; x += 256) lds[x] = 0u;
  ca.listed[tid] = ca.tomb[tid] = 0;
  ca.cmin[tid] = ca.hmax[tid] = ca.amax[tid] = -1;
  ca.sum[tid] = 0ull;
  if (tid < kBins) bh[tid] = 0ull;
  // which of the block's rows run (a bit per row, 16 rows per thread), so
  // that the walk decides from LDS and a stopped row costs no table read
  uint16_t* am = reinterpret_cast<uint16_t*>(bh + kBins);
  {
    uint32_t bits = 0u;
    for (int x = 0; x < 16; ++x) {
      const int64_t s = s0 + tid * 16 + x;
      if (s < s1 && d.alive[d.row0 + s] != 0) bits |= 1u << x;
    }
    am[tid] = (uint16_t)bits;
  }
  __syncthreads();

  // Per pair m of cells, one per 16-bit half. Tier: cells 2m (low) and 2m + 1
  // (high) are nibbles m and m + 4 of a word; code = the lag nibble, cmx1 =
  // the highest code + 1. 16-bit: the halves of word m; code = the offset
  // from the column's base, cmx1 = the highest offset.
  uint32_t ncnt[4], ntomb[4], cmin[4], cmx1[4], namax[4];
  uint32_t csum[8];  // code sums: tier [0..3] packed pairs, 16-bit one per cell
  // tier, per nibble, flushed into the pairs before a field can wrap: listed /
  // tombstoned cells (4-bit counters), code sums (8-bit, even and odd nibbles)
  uint32_t cacc = 0u, tacc = 0u, se = 0u, so = 0u;
  int nacc = 0;
  auto flush = [&]() {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      ncnt[m] += (cacc >> (4 * m)) & 0x000F000Fu;
      ntomb[m] += (tacc >> (4 * m)) & 0x000F000Fu;
      csum[m] += (((m & 1) ? so : se) >> (8 * (m >> 1))) & 0x00FF00FFu;
    }
    cacc = tacc = se = so = 0u;
    nacc = 0;
  };
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    ncnt[m] = ntomb[m] = cmx1[m] = namax[m] = 0u;
    cmin[m] = TIER ? 0x000F000Fu : 0x03FF03FFu;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) csum[j] = 0u;

  if (c < d.ncol) {
    const int64_t tcell = tile * d.tstride + q * 8;
    constexpr int UN = 4;  // rows in flight per lane
    for (int64_t sb = s0 + rsub; sb < s1; sb += UN * rstep) {
      bool run[UN];
      uint32_t aw[UN], uw[UN];
      uint4 xs[UN];
#pragma unroll
      for (int k = 0; k < UN; ++k) {
        const int64_t s = sb + k * rstep;
        const int64_t x = s - s0;
        run[k] = s < s1 && ((am[x >> 4] >> (x & 15)) & 1u) != 0;  // a stopped row has no view
        aw[k] = uw[k] = 0u;
        if (!run[k]) continue;
        const int64_t cell = tcell + (s << d.lgtw);
        if (TIER) {
          aw[k] = d.a4[cur][cell >> 3];
          uw[k] = d.pl[cur][cell >> 3];
        } else {
          xs[k] = *reinterpret_cast<const uint4*>(d.hn[cur] + cell);  // (gh_ld16s of a 16-bit buffer's owned slot)
        }
      }
      uint32_t escm = 0u;  // the rows whose chunk needs the decoder
#pragma unroll
      for (int k = 0; k < UN; ++k) {
        if (!run[k]) continue;
        const int64_t i = d.row0 + sb + k * rstep;
        const int jd = gh_jd(d, i, c);
        if (!TIER) {
          const uint32_t h0 = xs[k].x & 0xFFFFu;
          if (h0 == GH_N_WIDE || h0 == GH_N_FROZEN) {
            escm |= 1u << k;
            continue;
          }
          uint32_t w[4] = {xs[k].x, xs[k].y, xs[k].z, xs[k].w};
#pragma unroll
          for (int m = 0; m < 4; ++m)  // the row's own entry: as an absent cell
            if (jd >= 0 && (jd >> 1) == m) w[m] |= 0xFFFFu << (16 * (jd & 1));
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const uint32_t y = w[m];
            const uint32_t off = pk_lshr16(y, 5) & 0x03FF03FFu;
            const uint32_t np = pk_zero_mask(off ^ 0x03FF03FFu);  // offset 1023: absent or tombstone
            const uint32_t ab = pk_zero_mask(~y);                 // absent
            const uint32_t ov = off & ~np, av = y & 0x001F001Fu & ~np;
            ncnt[m] += ~np & 0x00010001u;
            ntomb[m] += np & ~ab & 0x00010001u;
            cmin[m] = pk_min_u16(cmin[m], off);
            cmx1[m] = pk_max_u16(cmx1[m], ov);
            namax[m] = pk_max_u16(namax[m], av);
            csum[2 * m] += ov & 0xFFFFu;
            csum[2 * m + 1] += ov >> 16;
            // a present narrow cell's age is its 5-bit field, exact
            atomicAdd(&hw[(av & 0xFFFFu) * 64], ~np & 1u);
            atomicAdd(&hw[(av >> 16) * 64], (~np >> 16) & 1u);
          }
          continue;
        }
        if (gh_t4_esc(aw[k])) {
          escm |= 1u << k;
          continue;
        }
        uint32_t u = uw[k], a = aw[k];
        if (jd >= 0) {  // the row's own entry: as an absent cell
          u |= 0xFu << gh_nib(jd);
          a |= 0xFu << gh_nib(jd);
        }
        // bit 0 of each nibble that is 15: a code 15 is not listed, and with
        // an age nibble other than 15 it is a tombstone
        uint32_t n15 = u & (u >> 1), a15 = a & (a >> 1);
        n15 &= (n15 >> 2) & 0x11111111u;
        a15 &= a15 >> 2;
        const uint32_t nvm = (n15 << 4) - n15;   // 0xF per nibble not listed
        const uint32_t uv = u & ~nvm, av = a & ~nvm;  // (their codes and ages as 0)
        cacc += n15 ^ 0x11111111u;
        tacc += n15 & ~a15;
        se += uv & 0x0F0F0F0Fu;
        so += (uv >> 4) & 0x0F0F0F0Fu;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const uint32_t U = (u >> (4 * m)) & 0x000F000Fu, A = (av >> (4 * m)) & 0x000F000Fu;
          cmin[m] = pk_min_u16(cmin[m], U);
          cmx1[m] = pk_max_u16(cmx1[m], (U + 0x00010001u) & 0x000F000Fu);  // (15 -> 0)
          namax[m] = pk_max_u16(namax[m], A);
          // a listed cell's age is its nibble (1..15); the others land in
          // bin 0, which no tier cell uses and this kernel's waves drop
          atomicAdd(&hw[(A & 0xFFFFu) * 64], 1u);
          atomicAdd(&hw[(A >> 16) * 64], 1u);
        }
      }
      if (TIER && ++nacc == 3) flush();  // 12 rows: counters <= 12, sums <= 180
      // the decoder's chunks: 16-bit codes of an escaped tier chunk, wide or
      // frozen cells, straight into the block's accumulators
      while (escm) {
        const int k = __builtin_ctz(escm);
        escm &= escm - 1u;
        const int64_t s = sb + k * rstep, i = d.row0 + s;
        const uint4 x = *reinterpret_cast<const uint4*>(d.hn[cur] + tcell + (s << d.lgtw));
        GhCell v[8];
        gh_dec8(d, cur, i, c, r, x, v);
        census_cells(d, i, c, r, v, bh, ca, cc0);
      }
    }
    // the lane's columns into the block's, as heartbeats: tier base +
    // GH_P_REF + 1 - code (the lowest code is the highest heartbeat), 16-bit
    // base + offset
    if (TIER) flush();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (c + j >= d.ncol) continue;
      const int m = j >> 1, sh = 16 * (j & 1);
      const int32_t n = (int32_t)((ncnt[m] >> sh) & 0xFFFFu), nt = (int32_t)((ntomb[m] >> sh) & 0xFFFFu);
      if (n) {
        const int32_t lo_c = (int32_t)((cmin[m] >> sh) & 0xFFFFu), hi_c = (int32_t)((cmx1[m] >> sh) & 0xFFFFu);
        const int32_t age = (int32_t)((namax[m] >> sh) & 0xFFFFu);
        if (TIER) {
          // (int64: with the owner at INT32_MAX - 1 or INT32_MAX, B itself is past int32)
          const int64_t B = (int64_t)d.base[cur][c + j] + GH_P_REF + 1;
          const int64_t sm = (int64_t)n * B - (int64_t)((csum[m] >> sh) & 0xFFFFu);
          ca.add(cc0 + j, n, (int32_t)(B + 1 - hi_c), (int32_t)(B - lo_c), (unsigned long long)sm, age);
        } else {
          const int32_t B = d.base[cur][c + j];
          const int64_t sm = (int64_t)n * B + (int64_t)csum[j];
          ca.add(cc0 + j, n, B + lo_c, B + hi_c, (unsigned long long)sm, age);
        }
      }
      if (nt) atomicAdd(&ca.tomb[cc0 + j], nt);
    }
  }
  __syncthreads();
  // the wave's bins (one column per lane) into the block's
  {
    const uint32_t* hb = lds + wave * (kBins * 64);
    unsigned long long mine = 0ull;
    for (int b = TIER ? 1 : 0; b < kBins; ++b) {
      uint32_t x = hb[b * 64 + lane];
      for (int w = 32; w > 0; w >>= 1) x += __shfl_xor(x, w);
      if (lane == b) mine = x;
    }
    if (lane < kBins && mine) atomicAdd(&bh[lane], mine);
  }
  __syncthreads();
  if (tid < kBins && bh[tid]) atomicAdd(&o.hist[tid], bh[tid]);
  const int64_t cg = tile * d.tw + tid;
  if (tid < d.tw && cg < d.ncol) {
    if (ca.listed[tid]) {
      atomicAdd(&o.listed[cg], ca.listed[tid]);
      atomicMax(&o.cmin[cg], ca.cmin[tid]);
      atomicMax(&o.hmax[cg], ca.hmax[tid]);
      atomicMax(&o.amax[cg], ca.amax[tid]);
      atomicAdd(&o.sum[cg], ca.sum[tid]);
    }
    if (ca.tomb[tid]) atomicAdd(&o.tomb[cg], ca.tomb[tid]);
  }
}

// Which of the two runs is the buffer's own flag (m8, device side): both are
// launched and the other returns at once, as the round variants do, so each
// walk is compiled to its own registers (4 waves per SIMD, which is also what
// the LDS admits: 4 workgroups per CU).
template <bool TIER>
__global__ __launch_bounds__(256, 4) void k_census(GhDev d, int cur, int32_t r, int64_t rpb, GhCensus o) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kHistWords + 5 * kColMax + 2 * kColMax + 2 * kBins + kRowsMax / 32];
  if (gh_m8(d, cur) != TIER) return;
  census_block<TIER>(d, cur, r, rpb, o, lds);
}

}  // namespace

void launch_census(const GhDev& d, int cur, int32_t r, const GhCensus& o, hipStream_t s) {
  if (d.nrows <= 0 || d.ncol <= 0) return;
  // row blocks: enough workgroups to fill the device, at least 64 rows each
  // (a block's LDS and global combine is paid once per block), at most 4,096
  // (the walk counts in 16-bit halves: rows per lane < 65,536 / 15)
  const int64_t rstep = 256 / (d.tw / 8);
  const int64_t want = std::max<int64_t>(1, GH_CENSUS_WGS / d.ntiles);
  int64_t rpb = std::max<int64_t>(64, (d.nrows + want - 1) / want);
  rpb = std::min<int64_t>((rpb + rstep - 1) / rstep * rstep, kRowsMax);
  const int64_t nrb = (d.nrows + rpb - 1) / rpb;
  const dim3 grid((unsigned)d.ntiles, (unsigned)nrb);
  if (d.a4[0]) hipLaunchKernelGGL(k_census<true>, grid, dim3(256), 0, s, d, cur, r, rpb, o);
  hipLaunchKernelGGL(k_census<false>, grid, dim3(256), 0, s, d, cur, r, rpb, o);
}
