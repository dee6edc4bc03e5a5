// mz_dqtab.hip — double Q-learning populations: the reference's DQAgent on the vectorised tabular
// engine of mz_qtab.hip (dense tables) and mz_qhash.hip (hashed tables).
//
// Reference (one env, one agent): DQAgent (agents/dq_agent.py:5-73) keeps two dicts of 4-entry
// float64 rows, q_a_values and q_b_values, and is driven by the same OffPolicyTrainer.train as
// QAgent. Per training step:
//   get_action (:35-46)  eps from steps_done, steps_done += 1, one draw: below eps a random action,
//                        else argmax Q_A[s]. Acting reads Q_A only.
//   update (:48-66)      one draw < 0.5 picks the table to update, A if true, B if false. In either
//                        case best = get_action(next_obs): a second eps-greedy choice on Q_A[s'],
//                        with eps from the already advanced steps_done, which it advances again
//                        (2 per training step, 1 per evaluation step). Updating A:
//                          td = reward + gamma * Q_B[s'][best] - Q_A[s][a]; Q_A[s][a] += lr * td
//                        updating B: the same with A and B swapped; best still comes from Q_A.
//                        There is no (not terminated) factor, and none here.
//   update_hyperparameter (:69-73) is QAgent's: the episode end of mz_qtab.h, reused as it is.
//
// Layout: a state's A row and B row sit side by side, [2][4] f64 = 64 B, 64-B aligned, so all an
// update reads of s' (the A row for the argmax, one element of A or B) is one 64-B segment.
//   dense   q    [T][rows][2][4]  (2.1 MB per table at 9x9)
//   hashed  keys int32 [T][C] exactly as mz_qhash.hip's (one key per state), vals [T][C][2][4]:
//           68 B per slot. One probe serves both tables; a write to either inserts the state's key.
//
// Per vector step:
//   k_dqtab_act / k_dqhash_act   qtab_choose on the A row with VectorQAgent's MZ_QTAB_STREAM draw;
//                    hashed acting never inserts. k_qtab_advance follows.
//   (mz_step)
//   k_dqtab_update / k_dqhash_update   independent tables, one launch. Draw
//                    mz_philox(seed, MZ_DQTAB_STREAM ^ (i << 32), ucounter): (w0 >> 8) * 2^-24 <
//                    0.5 -> update A; u2 = (w1 >> 8) * 2^-24 against eps from steps_done[t] as the
//                    update finds it (after the act's advance): u2 < eps -> best = w2 >> 30, else
//                    the first maximum of A[s']. Then the td, the store (hashed: find or insert; a
//                    full table drops the write and counts overflow) and the episode end. took[i]
//                    = 1 where a td was computed.
//   k_dqtab_td + k_dqtab_apply / k_dqhash_apply   shared tables: the read-only pass takes the coin,
//                    best and the td from the tables as they stood and writes lr * td and the
//                    chosen table per instance; the second pass does one f64 atomic add into the
//                    chosen table's element (hashed: claim by mz_qhash.h's CAS first), then
//                    qtab_end_atomic. Lookups and concurrent inserts never share a launch.
//   k_qtab_advance(table_of, took)   adds the inner get_actions to steps_done: a launch of its
//                    own, so that every lane of the update read the old value. An update dropped
//                    by a full table still counts its get_action.
// Launches per vector step (act, advance, env step, update, advance, reset): 6 independent,
// 7 shared.
//
// Overrides, for replaying the reference: coin (uint8 per instance, 0 = A, 1 = B) and next_action
// (int32 in 0..3) replace the draws; with next_action no eps is evaluated, steps_done still
// advances. A next_action outside 0..3 makes the instance idle for this update.
#include "../../include/mazerl.h"
#include "mz_qhash.h"
#include "mz_qtab.h"

namespace {

struct Row2 { Row a, b; };

__device__ inline Row2 dq_rows_at(const double* p8) {  // [2][4] f64 at a 64-B aligned address
  return Row2{qtab_row_at(p8), qtab_row_at(p8 + 4)};
}

constexpr Row ZERO_ROW{{0.0, 0.0, 0.0, 0.0}};

struct DenseFetch2 {
  const double* q;
  int64_t rows;
  __device__ Row2 operator()(int t, int64_t s) const {
    return dq_rows_at(q + ((int64_t)t * rows + s) * 8);
  }
};

// keeps the last probe (of s, after dqtab_td) for the store that follows
struct HashFetch2 {
  MzQhash h;
  int state;
  uint32_t slot;
  __device__ Row2 operator()(int t, int64_t s) {
    const int64_t base = (int64_t)t * h.C;
    state = qhash_probe(h.keys + base, h.C, h.shift, (int32_t)s, slot);
    if (state != QH_FOUND) return Row2{ZERO_ROW, ZERO_ROW};
    return dq_rows_at(h.vals + (base + slot) * 8);
  }
};

__global__ __launch_bounds__(QT_T) void k_dqtab_act(MzQtabAct a) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= a.n) return;
  const int t = qtab_act_table(a, i);
  if (t < 0) return;
  const int64_t s = qtab_index(a.obs6, i, a.P);
  qtab_choose(a, i, t, s, qtab_row_at(a.q + ((int64_t)t * a.rows + s) * 8));  // the A row
}

__global__ __launch_bounds__(QT_T) void k_dqhash_act(MzQtabAct a, MzQhash h) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= a.n) return;
  const int t = qtab_act_table(a, i);
  if (t < 0) return;
  const int64_t s = qtab_index(a.obs6, i, a.P);
  const int64_t base = (int64_t)t * h.C;
  uint32_t slot;
  const bool found = qhash_probe(h.keys + base, h.C, h.shift, (int32_t)s, slot) == QH_FOUND;
  qtab_choose(a, i, t, s, found ? qtab_row_at(h.vals + (base + slot) * 8) : ZERO_ROW);
}

// What one instance's update contributes: the element it updates and lr * td.
struct Td2 {
  int t, act, which;  // which: 0 = table A, 1 = table B
  int64_t s;
  double add, old;
};

// fetch(t, s) -> Row2, called for s' first and for s last (see mz_qtab.h's qtab_td).
template <class Fetch>
__device__ inline bool dqtab_td(const MzDqtabUpd& d, int i, Td2& o, Fetch&& fetch) {
  const MzQtabUpd& u = d.u;
  o.t = qtab_table(u.table_of, i, u.T);
  if (o.t < 0) return false;
  o.s = u.sidx[i];
  o.act = u.actions[i];
  if (o.s < 0 || o.s >= u.rows || (unsigned)o.act > 3u) return false;
  int best = d.next_action ? d.next_action[i] : 0;
  if ((unsigned)best > 3u) return false;
  const int64_t s2 = qtab_index(u.obs6, i, u.P);
  const Row2 nxt = fetch(o.t, s2);
  const Row2 cur = fetch(o.t, o.s);
  uint32_t w[4];
  mz_philox(d.seed, MZ_DQTAB_STREAM ^ ((uint64_t)(uint32_t)i << 32), d.ucounter, w);
  const bool to_a = d.coin ? d.coin[i] == 0 : (double)(w[0] >> 8) * (1.0 / 16777216.0) < 0.5;
  if (!d.next_action) {  // the inner get_action on Q_A[s']
    const double eps =
        qtab_eps(d.steps_done[o.t], d.eps_init[o.t], d.eps_final[o.t], d.eps_decay[o.t]);
    const double u2 = (double)(w[1] >> 8) * (1.0 / 16777216.0);
    best = u2 < eps ? (int)(w[2] >> 30) : qtab_argmax(nxt.a);
  }
  o.which = to_a ? 0 : 1;
  const double other = to_a ? qtab_pick(nxt.b, best) : qtab_pick(nxt.a, best);
  o.old = to_a ? qtab_pick(cur.a, o.act) : qtab_pick(cur.b, o.act);
  const double td = __dsub_rn(__dadd_rn(u.reward64[i], __dmul_rn(u.gamma[o.t], other)), o.old);
  o.add = __dmul_rn(u.lr[o.t], td);
  return true;
}

// independent tables (table_of NULL): nobody else touches instance i's tables, gamma or counters
__global__ __launch_bounds__(QT_T) void k_dqtab_update(MzDqtabUpd d) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= d.u.n) return;
  Td2 o;
  const bool ok = dqtab_td(d, i, o, DenseFetch2{d.u.q, d.u.rows});
  d.took[i] = ok;
  if (!ok) return;
  d.u.q[((int64_t)o.t * d.u.rows + o.s) * 8 + o.which * 4 + o.act] = __dadd_rn(o.old, o.add);
  qtab_end_plain(d.u, i, o.t);
}

// independent tables, hashed: lane i owns table i
__global__ __launch_bounds__(QT_T) void k_dqhash_update(MzDqtabUpd d, MzQhash h) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= d.u.n) return;
  Td2 o;
  HashFetch2 f{h, QH_FULL, 0u};
  const bool ok = dqtab_td(d, i, o, f);
  d.took[i] = ok;
  if (!ok) return;
  if (f.state == QH_FULL) {
    h.overflow[o.t] += 1;
  } else {
    const int64_t at = (int64_t)o.t * h.C + f.slot;
    if (f.state == QH_EMPTY) {
      h.keys[at] = (int32_t)o.s;
      h.load[o.t] += 1;
    }
    h.vals[at * 8 + o.which * 4 + o.act] = __dadd_rn(o.old, o.add);
  }
  qtab_end_plain(d.u, i, o.t);
}

// shared tables, pass 1 (either storage): read-only on the tables, gamma and steps_done
template <class Fetch>
__global__ __launch_bounds__(QT_T) void k_dqtab_td(MzDqtabUpd d, Fetch f) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= d.u.n) return;
  Td2 o;
  const bool ok = dqtab_td(d, i, o, f);
  d.took[i] = ok;
  d.which[i] = ok ? o.which : 0;
  d.u.td[i] = ok ? o.add : 0.0;
}

// shared tables, pass 2: one f64 atomic add into the chosen table's element, then the episode end
__global__ __launch_bounds__(QT_T) void k_dqtab_apply(MzDqtabUpd d) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= d.u.n || !d.took[i]) return;
  const MzQtabUpd& u = d.u;
  const int t = qtab_table(u.table_of, i, u.T);
  if (t < 0) return;
  const int64_t s = u.sidx[i];
  const int act = u.actions[i];
  if (s < 0 || s >= u.rows || (unsigned)act > 3u) return;
  unsafeAtomicAdd(u.q + ((int64_t)t * u.rows + s) * 8 + (d.which[i] ? 4 : 0) + act, u.td[i]);
  qtab_end_atomic(u, i, t);
}

// the same on hashed tables: find or insert first. Reads no row.
__global__ __launch_bounds__(QT_T) void k_dqhash_apply(MzDqtabUpd d, MzQhash h) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= d.u.n || !d.took[i]) return;
  const MzQtabUpd& u = d.u;
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
    unsafeAtomicAdd(h.vals + (base + slot) * 8 + (d.which[i] ? 4 : 0) + act, u.td[i]);
  } else {
    atomicAdd(reinterpret_cast<unsigned long long*>(h.overflow + t), 1ull);
  }
  qtab_end_atomic(u, i, t);
}

// k_qhash_rehash for the 64-B slot
__global__ __launch_bounds__(QT_T) void k_dqhash_rehash(MzQhash from, MzQhash to, int64_t total) {
  const int64_t stride = (int64_t)gridDim.x * QT_T;
  for (int64_t at = (int64_t)blockIdx.x * QT_T + threadIdx.x; at < total; at += stride) {
    const int32_t key = from.keys[at];
    if (key < 0) continue;
    const int t = (int)(at >> (32 - from.shift));
    const int64_t base = (int64_t)t * to.C;
    uint32_t slot;
    bool fresh;
    if (qhash_claim(to.keys + base, to.C, to.shift, key, slot, fresh)) {
      const double2* src = reinterpret_cast<const double2*>(from.vals + at * 8);
      double2* dst = reinterpret_cast<double2*>(to.vals + (base + slot) * 8);
#pragma unroll
      for (int k = 0; k < 4; ++k) dst[k] = src[k];
    } else {
      atomicAdd(reinterpret_cast<unsigned long long*>(to.overflow + t), 1ull);
    }
  }
}

// k_qhash_lookup for the 64-B slot: rows_out [m][2][4]
__global__ __launch_bounds__(QT_T) void k_dqhash_lookup(MzQhash h, int T, const int32_t* tables,
                                                        const int64_t* keys, int m,
                                                        double* rows_out, int32_t* slots_out) {
  const int j = blockIdx.x * QT_T + threadIdx.x;
  if (j >= m) return;
  const int t = tables[j];
  const int64_t key = keys[j];
  Row2 r{ZERO_ROW, ZERO_ROW};
  int32_t slot = -1;
  if ((unsigned)t < (unsigned)T && key >= 0 && key < (1ll << 31)) {
    HashFetch2 f{h, QH_FULL, 0u};
    r = f(t, key);
    if (f.state == QH_FOUND) slot = (int32_t)f.slot;
  }
  double2* o = reinterpret_cast<double2*>(rows_out + (size_t)j * 8);
  o[0] = double2{r.a.v[0], r.a.v[1]};
  o[1] = double2{r.a.v[2], r.a.v[3]};
  o[2] = double2{r.b.v[0], r.b.v[1]};
  o[3] = double2{r.b.v[2], r.b.v[3]};
  slots_out[j] = slot;
}

}  // namespace

hipError_t mz_launch_dqtab_act(const MzQtabAct& a, const MzQhash* h, long long* steps_done,
                               hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const dim3 grid((a.n + QT_T - 1) / QT_T), block(QT_T);
  if (h)
    hipLaunchKernelGGL(k_dqhash_act, grid, block, 0, s, a, *h);
  else
    hipLaunchKernelGGL(k_dqtab_act, grid, block, 0, s, a);
  return mz_launch_qtab_advance(a.table_of, a.active, a.n, a.T, steps_done, s);
}

hipError_t mz_launch_dqtab_update(const MzDqtabUpd& d, const MzQhash* h, long long* steps_done,
                                  hipStream_t s) {
  const MzQtabUpd& u = d.u;
  if (u.n <= 0) return hipSuccess;
  const dim3 grid((u.n + QT_T - 1) / QT_T), block(QT_T);
  if (!u.table_of) {
    if (h)
      hipLaunchKernelGGL(k_dqhash_update, grid, block, 0, s, d, *h);
    else
      hipLaunchKernelGGL(k_dqtab_update, grid, block, 0, s, d);
  } else if (h) {
    hipLaunchKernelGGL(k_dqtab_td<HashFetch2>, grid, block, 0, s, d, HashFetch2{*h, QH_FULL, 0u});
    hipLaunchKernelGGL(k_dqhash_apply, grid, block, 0, s, d, *h);
  } else {
    hipLaunchKernelGGL(k_dqtab_td<DenseFetch2>, grid, block, 0, s, d, DenseFetch2{u.q, u.rows});
    hipLaunchKernelGGL(k_dqtab_apply, grid, block, 0, s, d);
  }
  // the inner get_actions, after every lane above has read steps_done
  return mz_launch_qtab_advance(u.table_of, d.took, u.n, u.T, steps_done, s);
}

hipError_t mz_launch_dqhash_rehash(const MzQhash& from, const MzQhash& to, int T, hipStream_t s) {
  const int64_t total = (int64_t)T * from.C;
  if (total <= 0) return hipSuccess;
  const int64_t want = (total + QT_T - 1) / QT_T;
  const int blocks = (int)(want < QH_MAX_BLOCKS ? want : QH_MAX_BLOCKS);
  hipLaunchKernelGGL(k_dqhash_rehash, dim3(blocks), dim3(QT_T), 0, s, from, to, total);
  return hipGetLastError();
}

hipError_t mz_launch_dqhash_lookup(const MzQhash& h, int T, const int32_t* tables,
                                   const int64_t* keys, int m, double* rows_out,
                                   int32_t* slots_out, hipStream_t s) {
  if (m <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dqhash_lookup, dim3((m + QT_T - 1) / QT_T), dim3(QT_T), 0, s, h, T, tables,
                     keys, m, rows_out, slots_out);
  return hipGetLastError();
}
