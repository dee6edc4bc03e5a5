// mz_archive.hip — the explored-maze archive: keep the mazes an instance trained on, on the
// device, and put one back.
//
// Reference: the env appends every maze it trains on to `env.mazes` — the first one and each
// update_maze() replacement (simple_maze_env.py:34,91; simple_variable_maze_env.py:39,106) — and
// test(n, new=False) replays them one by one through update_visited_maze()
// (off_policy_trainer.py:84-119). Here a win overwrites the instance's tables, so the maze is
// kept as what it takes to rebuild them: its open cells as a bit field, the two meta words and
// the algorithm id (2 KB at 127 x 127 where the built tables take ~70 KB).
//
// The caller owns the archive memory (torch tensors): per instance a ring of `slots` entries,
//   bits [B][slots][W] int32, W = ceil(P * P / 32): bit (r N + c) & 31 of word (r N + c) >> 5 is
//                      1 iff cell (r, c) is open — row-major with the entry's own N, zero past N N;
//   meta [B][slots][2] the instance's meta0 / meta1 words (mz_common.h);
//   algo [B][slots]    its algorithm id;
//   count [B]          pushes so far: the next push goes to slot count % slots.
//
//   k_archive_push  one wave per instance: 64 cells per pass, their open bits (MZ_CELL_OPEN of
//                   the cell words) gathered by a wave ballot — two words per pass, lane k keeps
//                   the ballot of pass k — and stored 8 B per lane, 512 B per wave instruction.
//                   One writer per instance, no atomics; the handle's state is only read.
//   k_archive_push_pools  the same entry, appended in instance order to the pool of the
//                   instance's group (its own comment below): with one group the explored-maze
//                   pool of a whole population, mazerl.archive.MazePool (mz_archive_push_pool);
//                   with G groups one pool per learner of a population of learners,
//                   mazerl.archive.MazePoolSet (mz_archive_push_pools).
//   k_archive_load  one wave per target: validates the entry (nothing is stored for a bad one:
//                   it is counted in *errors), unpacks the bits into the build's LDS grid and
//                   runs the import branch of mz_build_one with the entry's own N — the launch of
//                   mz_load_mazes without its host copies and synchronisation, and with targets
//                   of different sizes in one launch.
#include "mz_archive.h"
#include "mz_build.inc.h"

#define WAVE 64
#define PUSH_WAVES 4  // instances (waves) per k_archive_push workgroup
#define POOL_SPAN 1024  // instances (threads) per k_archive_push_pool workgroup: 16 waves

namespace {

// One wave packs instance e into linear entry `ent` of [*, words] / [*, 2] / [*] arrays: the bit
// field by the ballot passes described above, then the meta words and the algorithm id by lane 0.
// Every lane of the wave must call it with the same (e, ent).
__device__ __forceinline__ void archive_pack_entry(const MzDev& d, int e, int lane, int words,
                                                   size_t ent, int32_t* __restrict__ bits,
                                                   int32_t* __restrict__ meta,
                                                   uint8_t* __restrict__ algo) {
  const uint32_t m0 = d.meta0[e], m1 = d.meta1[e];
  const int N = min((int)(m0 & 0xFF), d.P);
  const uint32_t* cells = d.cells + (size_t)e * d.P * d.P;
  uint2* out = reinterpret_cast<uint2*>(bits + ent * words);  // (8-B aligned only for even words)
  int32_t* outw = bits + ent * words;
  const bool wide = ((reinterpret_cast<uintptr_t>(outw) & 7u) == 0);
  const int passes = (words + 1) / 2;  // covers every word: the ones past N * N are stored as 0
  unsigned long long keep = 0ull;
  for (int p = 0; p < passes; ++p) {
    const int i = p * WAVE + lane;
    bool open = false;
    if (i < N * N) {
      const int r = i / N, c = i - r * N;
      open = (cells[r * d.P + c] & MZ_CELL_OPEN) != 0u;
    }
    const unsigned long long b = __ballot(open);
    if (lane == (p & (WAVE - 1))) keep = b;
    if ((p & (WAVE - 1)) == WAVE - 1 || p == passes - 1) {  // flush: lane k holds pass p0 + k
      const int p0 = p & ~(WAVE - 1), q = p0 + lane;
      if (q <= p) {
        const uint32_t lo = (uint32_t)keep, hi = (uint32_t)(keep >> 32);
        if (wide && 2 * q + 1 < words) {
          out[q] = make_uint2(lo, hi);
        } else {
          outw[2 * q] = (int32_t)lo;
          if (2 * q + 1 < words) outw[2 * q + 1] = (int32_t)hi;
        }
      }
      keep = 0ull;
    }
  }
  if (lane == 0) {
    meta[2 * ent] = (int32_t)m0;
    meta[2 * ent + 1] = (int32_t)m1;
    algo[ent] = d.algo[e];
  }
}

__global__ __launch_bounds__(WAVE * PUSH_WAVES) void k_archive_push(
    MzDev d, const uint8_t* __restrict__ flags, int slots, int words, int32_t* __restrict__ bits,
    int32_t* __restrict__ meta, uint8_t* __restrict__ algo, int32_t* __restrict__ count) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int e = blockIdx.x * PUSH_WAVES + (threadIdx.x >> 6);  // wave-uniform
  if (e >= d.B || (flags && !flags[e])) return;
  const uint32_t cnt = (uint32_t)count[e];
  const size_t ent = (size_t)e * slots + cnt % (uint32_t)slots;
  archive_pack_entry(d, e, lane, words, ent, bits, meta, algo);
  if (lane == 0) count[e] = (int32_t)(cnt + 1u);
}

// Nonzero bytes of a 32-bit word: bit 7 of each byte of y is set iff that byte of x is not 0.
__device__ __forceinline__ int nonzero_bytes(uint32_t x) {
  const uint32_t y = (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
  return __popc(y);
}

// k_archive_push_pools — G pools, one per group of b = B / G consecutive instances, each filled in
// instance order (G = 1: one pool for the whole population, mz_archive_push_pool).
//
// Group g has nblk = ceil(b / S) workgroups, S = POOL_SPAN; workgroup (g, k) = block g nblk + k
// owns the instances [g b + k S, min(g b + (k + 1) S, (g + 1) b)) and nothing of another group:
// with b < S one workgroup serves one small group (and is launched with ceil(b / 64) waves
// only). The slot of a flagged instance in pool g is c_g + (flagged instances of group g with a
// smaller id), so no workgroup waits for another:
//   1. the workgroup counts the nonzero flags of its group before its span itself (flags[g b ..
//      g b + k S): byte loads up to the first 16-B boundary — a group start need not be a multiple
//      of 16 — then 16-B loads, then the bytes left; at B = 65,536 at most 63 KB, out of L2) and
//      reduces the count over its waves through LDS;
//   2. it ranks its own flags by a wave ballot, popcount of the lanes below, and a table of the
//      wave counts in LDS, and writes the local ids of its flagged instances to an LDS list in
//      rank order;
//   3. its waves take list items in turn (wave w: items w, w + waves, ...), and pack item j into
//      entry c_g + prefix + j of pool g (row g capacity + that) when that is below `capacity`:
//      anything at or past it is dropped before any address is formed. Lane 0 adds owner — the
//      instance's id within its group — and stamp.
// flags == NULL: every instance is flagged, the prefix is k S and nothing is read for it.
//
// The counts. Each group has a two-word counter whose parity the caller keeps: `count_in[2 g]` is
// read by every workgroup of the group and written by none, the other word of the pair,
// `count_out[2 g]`, is written once, by the group's last workgroup (its prefix + its own flagged
// instances is |F_g|), as min(c_g + |F_g|, INT32_MAX). Nothing is exchanged between workgroups
// inside the launch — no atomic, no fence, no ticket — so the result cannot depend on the order
// in which they run, and two launches back to back on a stream are ordered by the stream alone:
// the second reads the words the first wrote.
__global__ __launch_bounds__(POOL_SPAN) void k_archive_push_pools(
    MzDev d, const uint8_t* __restrict__ flags, int b, int nblk, int capacity, int words,
    int32_t* __restrict__ bits, int32_t* __restrict__ meta, uint8_t* __restrict__ algo,
    int32_t* __restrict__ owner, int32_t* __restrict__ stamps, const int32_t* __restrict__ count_in,
    int32_t* __restrict__ count_out, int32_t stamp) {
  __shared__ int s_wave[POOL_SPAN / WAVE];      // per-wave partial sums, then per-wave flag counts
  __shared__ uint16_t s_list[POOL_SPAN];        // local ids of the flagged instances, in order
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  const int nthr = blockDim.x, nwav = nthr >> 6;  // (a multiple of 64, <= POOL_SPAN)
  const int g = blockIdx.x / nblk, k = blockIdx.x - g * nblk;
  const int gbase = g * b;                      // (< B <= INT32_MAX)
  const int off = k * POOL_SPAN;                // this span's first instance within the group (< b)
  // 1. flagged instances of this group before this span
  int before = off;
  if (flags) {
    const uint8_t* f = flags + gbase;           // f[0 .. off) lies inside the group
    int part = 0;
    const int head = min(off, (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(f) & 15u)) & 15u));
    const int body = (off - head) >> 4;         // whole 16-B words from the boundary on
    if (tid < head) part += f[tid] != 0;
    const uint4* f4 = reinterpret_cast<const uint4*>(f + head);
    for (int i = tid; i < body; i += nthr) {
      const uint4 v = f4[i];
      part += nonzero_bytes(v.x) + nonzero_bytes(v.y) + nonzero_bytes(v.z) + nonzero_bytes(v.w);
    }
    const int tail = head + (body << 4) + tid;  // (fewer than 16 bytes are left)
    if (tail < off) part += f[tail] != 0;
    for (int o = WAVE / 2; o > 0; o >>= 1) part += __shfl_down(part, o);
    if (lane == 0) s_wave[wave] = part;
    __syncthreads();
    before = 0;
    for (int w = 0; w < nwav; ++w) before += s_wave[w];
    __syncthreads();  // s_wave is reused below
  }
  // 2. rank this span's flags
  const int loc = off + tid;                    // id within the group
  const bool mine = loc < b && (!flags || flags[gbase + loc] != 0);
  const unsigned long long vote = __ballot(mine);
  if (lane == 0) s_wave[wave] = __popcll(vote);
  __syncthreads();
  int woff = 0, here = 0;
  for (int w = 0; w < nwav; ++w) {
    const int c = s_wave[w];
    if (w < wave) woff += c;
    here += c;
  }
  if (mine) s_list[woff + __popcll(vote & ((1ull << lane) - 1ull))] = (uint16_t)tid;
  __syncthreads();
  // 3. pack: one wave per list item (everything below is uniform per wave)
  const long long c0 = (long long)count_in[2 * g] + before;  // pool entry of this span's first item
  const size_t row0 = (size_t)g * (size_t)capacity;          // pool g's first row
  for (int j = wave; j < here; j += nwav) {
    const long long ent = c0 + j;
    if (ent >= capacity) break;  // dropped, and so is every later item of this wave
    const int local = off + (int)s_list[j];
    const size_t row = row0 + (size_t)ent;
    archive_pack_entry(d, gbase + local, lane, words, row, bits, meta, algo);
    if (lane == 0) {
      owner[row] = local;
      stamps[row] = stamp;
    }
  }
  if (k == nblk - 1 && tid == 0) {
    const long long total = (long long)count_in[2 * g] + before + here;
    count_out[2 * g] = (int32_t)(total > 0x7FFFFFFFll ? 0x7FFFFFFFll : total);
  }
}

// The launch of k_archive_push_pools: `groups` pools of `capacity` rows over the handle's B
// instances (B % groups == 0), group g reading count_in[2 g] and writing count_out[2 g].
hipError_t launch_push_pools(const MzDev& d, const uint8_t* flags, int groups, int capacity,
                             int words, int32_t* bits, int32_t* meta, uint8_t* algo,
                             int32_t* owner, int32_t* stamps, const int32_t* count_in,
                             int32_t* count_out, int32_t stamp, hipStream_t stream) {
  const int b = d.B / groups;
  const int nblk = (b + POOL_SPAN - 1) / POOL_SPAN;  // (groups nblk <= B)
  const int threads = b < POOL_SPAN ? (b + WAVE - 1) / WAVE * WAVE : POOL_SPAN;
  hipLaunchKernelGGL(k_archive_push_pools, dim3(groups * nblk), dim3(threads), 0, stream, d, flags,
                     b, nblk, capacity, words, bits, meta, algo, owner, stamps, count_in, count_out,
                     stamp);
  return hipGetLastError();
}

__global__ __launch_bounds__(WAVE) void k_archive_load(
    MzDev d, const int32_t* __restrict__ env_ids, int n, const int32_t* __restrict__ slot,
    int words, const int32_t* __restrict__ bits, const int32_t* __restrict__ meta,
    const uint8_t* __restrict__ algo, int32_t* errors) {
  extern __shared__ __align__(16) uint8_t lds[];
  const int lane = threadIdx.x;
  const MzBuildLds L = mz_build_lds(lds, d.P);
  for (int j = blockIdx.x; j < n; j += gridDim.x) {  // (everything below is uniform per wave)
    const int s = slot[j];
    if (s < 0) continue;  // leave this instance alone
    const int e = env_ids ? env_ids[j] : j;
    const uint32_t m0 = (uint32_t)meta[2 * (size_t)s], m1 = (uint32_t)meta[2 * (size_t)s + 1];
    const int N = (int)(m0 & 0xFF), W = (int)((m0 >> 8) & 0xFF);
    const int sr = (int)((m0 >> 16) & 0xFF), sc = (int)(m0 >> 24);
    const int gr = (int)(m1 & 0xFF), gc = (int)((m1 >> 8) & 0xFF);
    const int a = (int)algo[s];
    const uint32_t* b = reinterpret_cast<const uint32_t*>(bits) + (size_t)s * words;
    // the memory contract: every index the build forms below is bounded by these checks, before
    // any store — N fits the destination's pitch and the source row, start and goal lie inside N
    bool ok = e >= 0 && e < d.B && (N & 1) && N >= 5 && N <= d.P && W == N &&
              mz_archive_entry_words(N) <= words && sr < N && sc < N && gr < N && gc < N &&
              a >= 0 && a <= 2 && !(d.enrich && !d.toroidal && N < 15);
    if (ok) {
      const int ps = sr * N + sc, pg = gr * N + gc;
      ok = ((b[ps >> 5] >> (ps & 31)) & 1u) && ((b[pg >> 5] >> (pg & 31)) & 1u);
    }
    if (!ok) {
      if (lane == 0) atomicAdd(errors, 1);
      continue;
    }
    for (int i = lane; i < N * N; i += WAVE) L.g[i] = (uint8_t)((b[i >> 5] >> (i & 31)) & 1u);
    __syncthreads();
    if (lane == 0) {
      L.g[gr * N + gc] = 2;
      d.algo[e] = (uint8_t)a;
    }
    __syncthreads();
    // the import branch: its grid source is the LDS grid itself (the copy is then the identity)
    mz_build_one(d, e, d.toroidal, false, 0, 0, N, L.g, sr, sc, gr, gc, lds);
    __syncthreads();
  }
}

int hip_fail(hipError_t e) { return mz_fail_msg(MZ_EHIP, hipGetErrorString(e)); }

}  // namespace

extern "C" {

int mz_archive_words(int32_t max_dim, int32_t* words) {
  if (!words) return mz_fail_msg(MZ_EINVAL, "null argument");
  if (max_dim < 5 || max_dim > MZ_MAX_DIM) return mz_fail_msg(MZ_EINVAL, "max_dim outside [5, MZ_MAX_DIM]");
  *words = mz_archive_entry_words(max_dim);
  return MZ_OK;
}

int mz_archive_push(mz_handle* h, const uint8_t* flags_dev, int32_t slots, int32_t words,
                    int32_t* bits_dev, int32_t* meta_dev, uint8_t* algo_dev, int32_t* count_dev,
                    void* stream) {
  if (!h || !bits_dev || !meta_dev || !algo_dev || !count_dev)
    return mz_fail_msg(MZ_EINVAL, "null argument");
  const MzDev& d = mz_handle_dev(h);
  if (slots < 1) return mz_fail_msg(MZ_EINVAL, "slots must be >= 1");
  if (words != mz_archive_entry_words(d.P))
    return mz_fail_msg(MZ_EINVAL, "words must equal mz_archive_words(the handle's max_dim)");
  MzDeviceGuard g(mz_handle_device(h));
  hipLaunchKernelGGL(k_archive_push, dim3((d.B + PUSH_WAVES - 1) / PUSH_WAVES),
                     dim3(WAVE * PUSH_WAVES), 0, static_cast<hipStream_t>(stream), d, flags_dev,
                     slots, words, bits_dev, meta_dev, algo_dev, count_dev);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MZ_OK : hip_fail(e);
}

int mz_archive_pool_span(int32_t* span) {
  if (!span) return mz_fail_msg(MZ_EINVAL, "null argument");
  *span = POOL_SPAN;
  return MZ_OK;
}

int mz_archive_push_pool(mz_handle* h, const uint8_t* flags_dev, int32_t capacity, int32_t words,
                         int32_t* bits_dev, int32_t* meta_dev, uint8_t* algo_dev,
                         int32_t* owner_dev, int32_t* stamp_dev, int32_t* count_dev, int32_t stamp,
                         void* stream) {
  if (!h || !bits_dev || !meta_dev || !algo_dev || !owner_dev || !stamp_dev || !count_dev)
    return mz_fail_msg(MZ_EINVAL, "null argument");
  const MzDev& d = mz_handle_dev(h);
  if (capacity < 1) return mz_fail_msg(MZ_EINVAL, "capacity must be >= 1");
  if (words != mz_archive_entry_words(d.P))
    return mz_fail_msg(MZ_EINVAL, "words must equal mz_archive_words(the handle's max_dim)");
  const uintptr_t cin = reinterpret_cast<uintptr_t>(count_dev);
  if (cin & 3u) return mz_fail_msg(MZ_EINVAL, "count_dev must be 4-byte aligned");
  // the two-word counter: the other word of count_dev's 8-byte-aligned pair is written
  int32_t* cout = reinterpret_cast<int32_t*>(cin ^ 4u);
  MzDeviceGuard g(mz_handle_device(h));
  const hipError_t e = launch_push_pools(d, flags_dev, 1, capacity, words, bits_dev, meta_dev,
                                         algo_dev, owner_dev, stamp_dev,
                                         static_cast<const int32_t*>(count_dev), cout, stamp,
                                         static_cast<hipStream_t>(stream));
  return e == hipSuccess ? MZ_OK : hip_fail(e);
}

int mz_archive_push_pools(mz_handle* h, const uint8_t* flags_dev, int32_t groups, int32_t capacity,
                          int32_t words, int32_t* bits_dev, int32_t* meta_dev, uint8_t* algo_dev,
                          int32_t* owner_dev, int32_t* stamp_dev, int32_t* count_dev,
                          int32_t parity, int32_t stamp, void* stream) {
  if (!h || !bits_dev || !meta_dev || !algo_dev || !owner_dev || !stamp_dev || !count_dev)
    return mz_fail_msg(MZ_EINVAL, "null argument");
  const MzDev& d = mz_handle_dev(h);
  if (groups < 1) return mz_fail_msg(MZ_EINVAL, "groups must be >= 1");
  if (d.B % groups) return mz_fail_msg(MZ_EINVAL, "the handle's instances must divide into the groups");
  if (capacity < 1) return mz_fail_msg(MZ_EINVAL, "capacity must be >= 1");
  if (words != mz_archive_entry_words(d.P))
    return mz_fail_msg(MZ_EINVAL, "words must equal mz_archive_words(the handle's max_dim)");
  if (reinterpret_cast<uintptr_t>(count_dev) & 7u)
    return mz_fail_msg(MZ_EINVAL, "count_dev must be 8-byte aligned");
  if (parity != 0 && parity != 1) return mz_fail_msg(MZ_EINVAL, "parity must be 0 or 1");
  MzDeviceGuard g(mz_handle_device(h));
  const hipError_t e = launch_push_pools(d, flags_dev, groups, capacity, words, bits_dev, meta_dev,
                                         algo_dev, owner_dev, stamp_dev, count_dev + parity,
                                         count_dev + (parity ^ 1), stamp,
                                         static_cast<hipStream_t>(stream));
  return e == hipSuccess ? MZ_OK : hip_fail(e);
}

int mz_archive_load(mz_handle* h, const int32_t* env_ids_dev, int32_t n, const int32_t* slot_dev,
                    int32_t words, const int32_t* bits_dev, const int32_t* meta_dev,
                    const uint8_t* algo_dev, int32_t* errors_dev, void* stream) {
  if (!h || !slot_dev || !bits_dev || !meta_dev || !algo_dev || !errors_dev)
    return mz_fail_msg(MZ_EINVAL, "null argument");
  const MzDev& d = mz_handle_dev(h);
  if (n < 0 || (!env_ids_dev && n > d.B)) return mz_fail_msg(MZ_EINVAL, "n out of range");
  if (words < 1) return mz_fail_msg(MZ_EINVAL, "words must be >= 1");
  if (n == 0) return MZ_OK;
  MzDeviceGuard g(mz_handle_device(h));
  // LDS and grid as mz_launch_build sizes an import (k_build): the square-grid build region of
  // the destination's pitch, one wave per target, persistent over the list
  const size_t lds = mz_import_lds(d.P, d.toroidal != 0);
  const hipError_t ae = mz_build_lds_attr(reinterpret_cast<const void*>(k_archive_load), lds);
  if (ae != hipSuccess) return hip_fail(ae);
  const int grid = mz_build_launch_grid(n, lds);
  hipLaunchKernelGGL(k_archive_load, dim3(grid), dim3(WAVE), lds, static_cast<hipStream_t>(stream),
                     d, env_ids_dev, n, slot_dev, words, bits_dev, meta_dev, algo_dev, errors_dev);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MZ_OK : hip_fail(e);
}

}  // extern "C"
