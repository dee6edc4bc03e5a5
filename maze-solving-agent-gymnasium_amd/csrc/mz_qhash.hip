// mz_qhash.hip — the vectorised tabular learner of mz_qtab.hip on hashed tables.
//
// Reference: QAgent (agents/q_agent.py:8-79) keeps a defaultdict(lambda: np.zeros(4)) that holds
// only the states an agent has met. A dense table (mz_qtab.hip) has 5 P^4 rows — 1.05 MB at 9x9
// but 452 MB at 41x41 and 6.9 GB at 81x81, of which a learner writes at most one row per step. Here
// a table is the reference's sparse structure: an open-addressing hash table in HBM.
//
// Storage, for T tables of capacity C (a power of two, 16 <= C <= 2^30, the same for all):
//   keys     int32 [T][C]     the dense state index of mz_qtab.h's qtab_index, -1 = empty. The
//                             index is < 5 * 127^4 < 2^31 for every legal pitch (asserted below).
//   vals     f64   [T][C][4]  zero-filled: a slot's row is the reference's fresh np.zeros(4) until
//                             it is written, and an absent key reads as that zero row.
//   load     int32 [T]        occupied slots
//   overflow int64 [T]        updates dropped because the table was full
// Keys and rows are separate arrays: linear probing scans consecutive 4-B keys, 32 to a 128-B
// line, so a probe chain normally costs one line of keys plus one 32-B row gather.
//
// Probe: slot0 = (uint32(key) * 0x9E3779B1u) >> (32 - log2 C), then +1 mod C. Every probe loop
// runs at most C iterations, so a full table terminates: a lookup then answers "absent", an
// update is dropped and counted in overflow[t] (its episode-end bookkeeping still runs). Keys are
// never deleted, so a chain ends at the first empty slot.
//
// Launches (everything but the row fetch / store is mz_qtab.h's, shared with the dense storage):
//   k_qhash_act      k_qtab_act with the row fetched by lookup: read-only, absent -> zeros, never
//                    inserts. sidx is the dense key acted from. k_qtab_advance follows, unchanged.
//   k_qhash_update   independent tables: look up s' and s, td, find or insert s, store
//                    old + lr * td (the key is inserted on every write, also of a zero value);
//                    plain loads and stores: lane i owns table i.
//   k_qhash_td + k_qhash_apply   shared tables: the read-only td pass, then find-or-insert and one
//                    f64 atomic add. A slot is claimed with a 32-bit atomicCAS(-1 -> key); the CAS
//                    returns the slot's key as it stands, so a lane that loses uses the slot if it
//                    now holds its own key and probes on otherwise. A slot's row is zero before the
//                    claim, so claim-then-add needs no further ordering. The plain key load in
//                    front of the CAS may be stale, but only as -1 (a key changes once, from -1,
//                    and never again), and then the CAS decides.
//   k_qhash_rehash   one lane per old slot re-inserts (key, row) into fresh arrays of another
//                    capacity with the same claim; load carries over.
//   k_qhash_lookup   rows (zeros if absent) and slots (-1 if absent) of m (table, key) pairs.
//
// Invariant the design rests on: lookups and inserts never run in the same launch on one table
// that several lanes share. Only k_qhash_apply and k_qhash_rehash insert concurrently, and neither
// reads any row of the table it inserts into; k_qhash_update inserts into a table no other lane
// touches, after its own two lookups.
#include "../../include/mazerl.h"
#include "mz_qhash.h"
#include "mz_qtab.h"

static_assert(5ll * MZ_MAX_DIM * MZ_MAX_DIM * MZ_MAX_DIM * MZ_MAX_DIM < (1ll << 31),
              "a dense state index must fit the int32 key");

namespace {

// The storage's row fetch for mz_qtab.h; keeps the last probe (of s, after qtab_td).
struct HashFetch {
  MzQhash h;
  int state;
  uint32_t slot;
  __device__ Row operator()(int t, int64_t s) {
    const int64_t base = (int64_t)t * h.C;
    state = qhash_probe(h.keys + base, h.C, h.shift, (int32_t)s, slot);
    if (state != QH_FOUND) return Row{{0.0, 0.0, 0.0, 0.0}};
    return qtab_row_at(h.vals + (base + slot) * 4);
  }
};

__global__ __launch_bounds__(QT_T) void k_qhash_act(MzQtabAct a, MzQhash h) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= a.n) return;
  const int t = qtab_act_table(a, i);
  if (t < 0) return;
  const int64_t s = qtab_index(a.obs6, i, a.P);
  HashFetch f{h, QH_FULL, 0u};
  qtab_choose(a, i, t, s, f(t, s));
}

// independent tables (table_of NULL): lane i owns table i
__global__ __launch_bounds__(QT_T) void k_qhash_update(MzQtabUpd u, MzQhash h) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= u.n) return;
  Td d;
  HashFetch f{h, QH_FULL, 0u};
  if (!qtab_td(u, i, d, f)) return;
  if (f.state == QH_FULL) {
    h.overflow[d.t] += 1;
  } else {
    const int64_t at = (int64_t)d.t * h.C + f.slot;
    if (f.state == QH_EMPTY) {
      h.keys[at] = (int32_t)d.s;
      h.load[d.t] += 1;
    }
    h.vals[at * 4 + d.act] = __dadd_rn(d.old, d.add);
  }
  qtab_end_plain(u, i, d.t);
}

// shared tables, pass 1: read-only on the table and on gamma
__global__ __launch_bounds__(QT_T) void k_qhash_td(MzQtabUpd u, MzQhash h) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= u.n) return;
  Td d;
  HashFetch f{h, QH_FULL, 0u};
  u.td[i] = qtab_td(u, i, d, f) ? d.add : 0.0;
}

// shared tables, pass 2: find or insert, one f64 atomic add, then the episode end. Reads no row.
__global__ __launch_bounds__(QT_T) void k_qhash_apply(MzQtabUpd u, MzQhash h) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= u.n) return;
  const int t = qtab_table(u.table_of, i, u.T);
  if (t < 0) return;
  const int64_t s = u.sidx[i];
  const int act = u.actions[i];
  if (s < 0 || s >= u.rows || (unsigned)act > 3u) return;
  const int64_t base = (int64_t)t * h.C;
  uint32_t slot;
  bool fresh;
  if (qhash_claim(h.keys + base, h.C, h.shift, (int32_t)s, slot, fresh)) {
    if (fresh) atomicAdd(h.load + t, 1);
    unsafeAtomicAdd(h.vals + (base + slot) * 4 + act, u.td[i]);
  } else {
    atomicAdd(reinterpret_cast<unsigned long long*>(h.overflow + t), 1ull);
  }
  qtab_end_atomic(u, i, t);
}

// One lane per old slot; the old capacity is 2^(32 - from.shift). An entry that finds the new
// table full is dropped and counted (the caller sizes the new table above the load).
__global__ __launch_bounds__(QT_T) void k_qhash_rehash(MzQhash from, MzQhash to, int64_t total) {
  const int64_t stride = (int64_t)gridDim.x * QT_T;
  for (int64_t at = (int64_t)blockIdx.x * QT_T + threadIdx.x; at < total; at += stride) {
    const int32_t key = from.keys[at];
    if (key < 0) continue;
    const int t = (int)(at >> (32 - from.shift));
    const int64_t base = (int64_t)t * to.C;
    uint32_t slot;
    bool fresh;
    if (qhash_claim(to.keys + base, to.C, to.shift, key, slot, fresh)) {
      const double2* src = reinterpret_cast<const double2*>(from.vals + at * 4);
      double2* dst = reinterpret_cast<double2*>(to.vals + (base + slot) * 4);
      dst[0] = src[0];
      dst[1] = src[1];
    } else {
      atomicAdd(reinterpret_cast<unsigned long long*>(to.overflow + t), 1ull);
    }
  }
}

__global__ __launch_bounds__(QT_T) void k_qhash_lookup(MzQhash h, int T, const int32_t* tables,
                                                       const int64_t* keys, int m,
                                                       double* rows_out, int32_t* slots_out) {
  const int j = blockIdx.x * QT_T + threadIdx.x;
  if (j >= m) return;
  const int t = tables[j];
  const int64_t key = keys[j];
  Row r{{0.0, 0.0, 0.0, 0.0}};
  int32_t slot = -1;
  if ((unsigned)t < (unsigned)T && key >= 0 && key < (1ll << 31)) {
    HashFetch f{h, QH_FULL, 0u};
    r = f(t, key);
    if (f.state == QH_FOUND) slot = (int32_t)f.slot;
  }
  double2* o = reinterpret_cast<double2*>(rows_out + (size_t)j * 4);
  o[0] = double2{r.v[0], r.v[1]};
  o[1] = double2{r.v[2], r.v[3]};
  slots_out[j] = slot;
}

}  // namespace

hipError_t mz_launch_qhash_act(const MzQtabAct& a, const MzQhash& h, long long* steps_done,
                               hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_qhash_act, dim3((a.n + QT_T - 1) / QT_T), dim3(QT_T), 0, s, a, h);
  return mz_launch_qtab_advance(a.table_of, a.active, a.n, a.T, steps_done, s);
}

hipError_t mz_launch_qhash_update(const MzQtabUpd& u, const MzQhash& h, hipStream_t s) {
  if (u.n <= 0) return hipSuccess;
  const int blocks = (u.n + QT_T - 1) / QT_T;
  if (!u.table_of) {
    hipLaunchKernelGGL(k_qhash_update, dim3(blocks), dim3(QT_T), 0, s, u, h);
  } else {
    hipLaunchKernelGGL(k_qhash_td, dim3(blocks), dim3(QT_T), 0, s, u, h);
    hipLaunchKernelGGL(k_qhash_apply, dim3(blocks), dim3(QT_T), 0, s, u, h);
  }
  return hipGetLastError();
}

hipError_t mz_launch_qhash_rehash(const MzQhash& from, const MzQhash& to, int T, hipStream_t s) {
  const int64_t total = (int64_t)T * from.C;
  if (total <= 0) return hipSuccess;
  const int64_t want = (total + QT_T - 1) / QT_T;
  const int blocks = (int)(want < QH_MAX_BLOCKS ? want : QH_MAX_BLOCKS);
  hipLaunchKernelGGL(k_qhash_rehash, dim3(blocks), dim3(QT_T), 0, s, from, to, total);
  return hipGetLastError();
}

hipError_t mz_launch_qhash_lookup(const MzQhash& h, int T, const int32_t* tables,
                                  const int64_t* keys, int m, double* rows_out, int32_t* slots_out,
                                  hipStream_t s) {
  if (m <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_qhash_lookup, dim3((m + QT_T - 1) / QT_T), dim3(QT_T), 0, s, h, T, tables,
                     keys, m, rows_out, slots_out);
  return hipGetLastError();
}
