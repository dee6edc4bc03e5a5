// mz_qtab.hip — config 1 vectorised: populations of tabular learners whose tables live in HBM.
// Q-learning and double Q-learning, on dense or hashed tables: every stage is one kernel template
// over a storage and a rule (mz_qtab.h).
//
// ---- Q-learning ----------------------------------------------------------------------------------
// Reference (one env, one agent): QAgent (agents/q_agent.py:8-79) keeps a dict of 4-entry float64
// rows keyed by str(obs); OffPolicyTrainer.train (lib/trainers/off_policy_trainer.py:28-80) runs
// get_action / env.step / update per step and, per episode, update_hyperparameter(cumulative > 0)
// (prev_cum_rew is zeroed at the top of every episode, :32, so :77 compares against 0).
//
// Vectorised (agents/vector_q.py, trainers/vector_tabular.py): n instances step together, one lane
// each, on the plain observation (r, c, gr, gc, br, bc) that k_step leaves in obs6 (write_obs6<false>,
// exact small integers in f32). Instance i learns on table t = table_of[i] (NULL: t = i).
//
// State index (mz_qtab_index, mirrored by VectorQAgent.state_index): a dense row
//   (((r * P + c) * P + gr) * P + gc) * 5 + k,  P = max_dim,  rows = 5 P^4 per table,
// k = the best-dir class: 0 none (0, 0), 1 down, 2 up, 3 right, 4 left — the move that leads to the
// best next cell ("best dir" = agent - best_next_cell, base_maze_env.py:122). On the torus the
// difference of a wrapped move is +-(N - 1) instead of -+1, so |x| > 1 is classified as the wrapped
// neighbour: br = -1 or br > 1 is down, br = 1 or br < -1 is up (columns alike). At a given agent
// cell the four moves give four different (br, bc), so two observations of one env share a row
// iff their str(obs) keys are equal. A row is 4 f64 = 32 B, read with two 16-B loads.
//
// Per vector step:
//   k_qtab_act      eps = final + (init - final) * exp(-1.0 * steps_done[t] / decay) in f64, one
//                   Philox draw per instance: u = (w0 >> 8) * 2^-24 < eps -> action w1 >> 30
//                   (action_space.sample(), uniform over 4 — not mz_act's masked distribution),
//                   else the row's first maximum (np.argmax). Writes the action and the row index.
//                   Instances masked out by `active` idle: action -1, no draw counted.
//   k_qtab_advance  steps_done[t] += the instances acting on t (one get_action each), after every
//                   lane of k_qtab_act has read it.
//   (mz_step)       the env step.
//   k_qtab_update   independent tables: future = terminated ? 0 : max(Q[s']),
//                   td = (reward + gamma * future) - Q[s][a], Q[s][a] = Q[s][a] + lr * td, then the
//                   episode end (gamma +- eta, counters).
//   k_qtab_td + k_qtab_apply   shared tables: the same td from the table as it stood before the
//                   step (a read-only pass writes lr * td per instance), then one native f64
//                   global atomic add per instance; colliding updates add. With one instance per
//                   row this gives the bits of the single pass (Q + lr * td is one f64 add either
//                   way). gamma and the counters take atomic adds as well.
// Shared-table determinism: colliding adds and the +-eta adds to gamma arrive in no fixed order,
// so results are bitwise reproducible only where the addends commute exactly (disjoint rows;
// equal addends); otherwise they can differ in the last bits from run to run.
//
// ---- hashed tables (Hashed<W>, mz_qhash.h) -------------------------------------------------------
// Reference: QAgent keeps a defaultdict(lambda: np.zeros(4)) that holds only the states an agent
// has met. A dense table has 5 P^4 rows — 1.05 MB at 9x9 but 452 MB at 41x41 and 6.9 GB at 81x81,
// of which a learner writes at most one row per step. A hashed table is the reference's sparse
// structure: an open-addressing hash table in HBM.
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
// What the stages do on hashed tables:
//   k_qtab_act       the row is fetched by lookup: read-only, absent -> zeros, never inserts. sidx
//                    is the dense key acted from. k_qtab_advance follows, unchanged.
//   k_qtab_update    independent tables: look up s' and s, td, find or insert s, store
//                    old + lr * td (the key is inserted on every write, also of a zero value);
//                    plain loads and stores: lane i owns table i.
//   k_qtab_td + k_qtab_apply   shared tables: the read-only td pass, then find-or-insert and one
//                    f64 atomic add. A slot is claimed with a 32-bit atomicCAS(-1 -> key); the CAS
//                    returns the slot's key as it stands, so a lane that loses uses the slot if it
//                    now holds its own key and probes on otherwise. A slot's row is zero before the
//                    claim, so claim-then-add needs no further ordering. The plain key load in
//                    front of the CAS may be stale, but only as -1 (a key changes once, from -1,
//                    and never again), and then the CAS decides.
//   k_qtab_rehash    one lane per old slot re-inserts (key, row) into fresh arrays of another
//                    capacity with the same claim; load carries over.
//   k_qtab_lookup    rows (zeros if absent) and slots (-1 if absent) of m (table, key) pairs.
//
// Invariant the design rests on: lookups and inserts never run in the same launch on one table
// that several lanes share. Only k_qtab_apply and k_qtab_rehash insert concurrently, and neither
// reads any row of the table it inserts into; k_qtab_update inserts into a table no other lane
// touches, after its own two lookups.
//
// ---- double Q-learning (RuleDQ, W = 2) -----------------------------------------------------------
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
//   hashed  keys int32 [T][C] exactly as Q-learning's (one key per state), vals [T][C][2][4]:
//           68 B per slot. One probe serves both tables; a write to either inserts the state's key.
//
// Per vector step:
//   k_qtab_act       qtab_choose on the A row with VectorQAgent's MZ_QTAB_STREAM draw; hashed
//                    acting never inserts. k_qtab_advance follows.
//   (mz_step)
//   k_qtab_update    independent tables, one launch. Draw
//                    mz_philox(seed, MZ_DQTAB_STREAM ^ (i << 32), ucounter): (w0 >> 8) * 2^-24 <
//                    0.5 -> update A; u2 = (w1 >> 8) * 2^-24 against eps from steps_done[t] as the
//                    update finds it (after the act's advance): u2 < eps -> best = w2 >> 30, else
//                    the first maximum of A[s']. Then the td, the store (hashed: find or insert; a
//                    full table drops the write and counts overflow) and the episode end. took[i]
//                    = 1 where a td was computed.
//   k_qtab_td + k_qtab_apply   shared tables: the read-only pass takes the coin, best and the td
//                    from the tables as they stood and writes lr * td and the chosen table per
//                    instance; the second pass does one f64 atomic add into the chosen table's
//                    element (hashed: claim by mz_qhash.h's CAS first), then qtab_end_atomic.
//                    Lookups and concurrent inserts never share a launch.
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
#include "mz_qtab.h"

static_assert(5ll * MZ_MAX_DIM * MZ_MAX_DIM * MZ_MAX_DIM * MZ_MAX_DIM < (1ll << 31),
              "a dense state index must fit the int32 key");

namespace {

// Row 0 alone is read: double Q acts on Q_A.
template <class S>
__global__ __launch_bounds__(QT_T) void k_qtab_act(MzQtabAct a, S st) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= a.n) return;
  const int t = qtab_act_table(a, i);
  if (t < 0) return;  // idle or no table: observe only
  const int64_t s = qtab_index(a.obs6, i, a.P);
  qtab_choose(a, i, t, s, st.row(st.find(t, s), 0));
}

// steps_done[t] += 1 per acting instance. A wave whose lanes share lane 0's table adds their count
// with one atomic (a shared table would otherwise take n atomics on one word).
__global__ __launch_bounds__(QT_T) void k_qtab_advance(const int32_t* table_of,
                                                       const uint8_t* active, int n, int T,
                                                       long long* steps_done) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= n || (active && !active[i])) return;
  const int t = qtab_table(table_of, i, T);
  if (t < 0) return;
  if (!table_of) {
    steps_done[t] += 1;
    return;
  }
  const int t0 = __builtin_amdgcn_readfirstlane(t);
  const unsigned long long same = __ballot(t == t0);
  if (t == t0) {
    const int lane = threadIdx.x & 63;
    if ((same & ((1ull << lane) - 1ull)) == 0ull)
      atomicAdd(reinterpret_cast<unsigned long long*>(steps_done + t0),
                (unsigned long long)__popcll(same));
  } else {
    atomicAdd(reinterpret_cast<unsigned long long*>(steps_done + t), 1ull);
  }
}

// independent tables (table_of NULL): nobody else touches instance i's table, gamma or counters
template <class R, class S>
__global__ __launch_bounds__(QT_T) void k_qtab_update(typename R::Args a, S st) {
  const MzQtabUpd& u = R::upd(a);
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= u.n) return;
  Td o;
  typename S::Loc at;
  const bool ok = R::td(a, i, o, st, at);
  R::set_took(a, i, ok);
  if (!ok) return;
  st.store(at, o.t, o.s, o.which * 4 + o.act, __dadd_rn(o.old, o.add));
  qtab_end_plain(u, i, o.t);
}

// shared tables, pass 1: read-only on the tables, gamma and steps_done
template <class R, class S>
__global__ __launch_bounds__(QT_T) void k_qtab_td(typename R::Args a, S st) {
  const MzQtabUpd& u = R::upd(a);
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= u.n) return;
  Td o;
  typename S::Loc at;
  const bool ok = R::td(a, i, o, st, at);
  R::set_took(a, i, ok);
  R::set_which(a, i, ok ? o.which : 0);
  u.td[i] = ok ? o.add : 0.0;
}

// shared tables, pass 2: one f64 atomic add per instance (hashed: find or insert first), then the
// episode end. Reads no row. Only lr * td (and the rule's took / which) comes over from pass 1, so
// the pass finds the instance's table, row and action again, under the same guard (qtab_who); the
// single-pass update has them from its td and does not look twice. took: a double-Q lane that
// pass 1 refused (also for a next_action outside 0..3, which the guard does not see) sits this out.
template <class R, class S>
__global__ __launch_bounds__(QT_T) void k_qtab_apply(typename R::Args a, S st) {
  const MzQtabUpd& u = R::upd(a);
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= u.n || !R::took(a, i)) return;
  int t, act;
  int64_t s;
  if (!qtab_who(u, i, t, s, act)) return;
  st.add(t, s, R::which(a, i) * 4 + act, u.td + i);
  qtab_end_atomic(u, i, t);
}

// One lane per old slot; the old capacity is 2^(32 - from.shift). An entry that finds the new
// table full is dropped and counted (the caller sizes the new table above the load).
template <int W>
__global__ __launch_bounds__(QT_T) void k_qtab_rehash(MzQhash from, MzQhash to, int64_t total) {
  const int64_t stride = (int64_t)gridDim.x * QT_T;
  for (int64_t at = (int64_t)blockIdx.x * QT_T + threadIdx.x; at < total; at += stride) {
    const int32_t key = from.keys[at];
    if (key < 0) continue;
    const int t = (int)(at >> (32 - from.shift));
    const int64_t base = (int64_t)t * to.C;
    uint32_t slot;
    bool fresh;
    if (qhash_claim(to.keys + base, to.C, to.shift, key, slot, fresh)) {
      const double2* src = reinterpret_cast<const double2*>(from.vals + at * (4 * W));
      double2* dst = reinterpret_cast<double2*>(to.vals + (base + slot) * (4 * W));
#pragma unroll
      for (int k = 0; k < 2 * W; ++k) dst[k] = src[k];
    } else {
      atomicAdd(reinterpret_cast<unsigned long long*>(to.overflow + t), 1ull);
    }
  }
}

// rows_out [m][W][4]
template <int W>
__global__ __launch_bounds__(QT_T) void k_qtab_lookup(Hashed<W> st, int T, const int32_t* tables,
                                                      const int64_t* keys, int m,
                                                      double* rows_out, int32_t* slots_out) {
  const int j = blockIdx.x * QT_T + threadIdx.x;
  if (j >= m) return;
  const int t = tables[j];
  const int64_t key = keys[j];
  typename Hashed<W>::Loc l{0, 0u, QH_FULL};  // reads as absent
  if ((unsigned)t < (unsigned)T && key >= 0 && key < (1ll << 31)) l = st.find(t, key);
  double2* o = reinterpret_cast<double2*>(rows_out + (size_t)j * (4 * W));
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const Row r = st.row(l, k);
    o[2 * k] = double2{r.v[0], r.v[1]};
    o[2 * k + 1] = double2{r.v[2], r.v[3]};
  }
  slots_out[j] = l.state == QH_FOUND ? (int32_t)l.slot : -1;
}

// f(rule, storage) for width (1: Q, 2: double Q) on q [T][rows][width][4], or on *h if there is one
template <class F>
void qtab_with(int width, const double* q, int64_t rows, const MzQhash* h, F&& f) {
  double* qw = const_cast<double*>(q);  // (acting only reads)
  if (width == 2) {
    if (h) f(RuleDQ{}, Hashed<2>{*h}); else f(RuleDQ{}, Dense<2>{qw, rows});
  } else {
    if (h) f(RuleQ{}, Hashed<1>{*h}); else f(RuleQ{}, Dense<1>{qw, rows});
  }
}

inline dim3 qtab_grid(int64_t lanes) { return dim3((unsigned)((lanes + QT_T - 1) / QT_T)); }

}  // namespace

hipError_t mz_launch_qtab_advance(const int32_t* table_of, const uint8_t* active, int n, int T,
                                  long long* steps_done, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_qtab_advance, qtab_grid(n), dim3(QT_T), 0, s, table_of, active, n, T,
                     steps_done);
  return hipGetLastError();
}

hipError_t mz_launch_qtab_act(const MzQtabAct& a, int width, const MzQhash* h,
                              long long* steps_done, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  qtab_with(width, a.q, a.rows, h, [&](auto, auto st) {
    hipLaunchKernelGGL(k_qtab_act<decltype(st)>, qtab_grid(a.n), dim3(QT_T), 0, s, a, st);
  });
  return mz_launch_qtab_advance(a.table_of, a.active, a.n, a.T, steps_done, s);
}

hipError_t mz_launch_qtab_update(const MzDqtabUpd& d, int width, const MzQhash* h,
                                 long long* steps_done, hipStream_t s) {
  const MzQtabUpd& u = d.u;
  if (u.n <= 0) return hipSuccess;
  qtab_with(width, u.q, u.rows, h, [&](auto rule, auto st) {
    using R = decltype(rule);
    using S = decltype(st);
    const typename R::Args& a = R::of(d);
    const dim3 grid = qtab_grid(u.n), block(QT_T);
    if (!u.table_of) {
      hipLaunchKernelGGL((k_qtab_update<R, S>), grid, block, 0, s, a, st);
    } else {
      hipLaunchKernelGGL((k_qtab_td<R, S>), grid, block, 0, s, a, st);
      hipLaunchKernelGGL((k_qtab_apply<R, S>), grid, block, 0, s, a, st);
    }
  });
  if (width != 2) return hipGetLastError();
  // double Q's inner get_actions, after every lane above has read steps_done
  return mz_launch_qtab_advance(u.table_of, d.took, u.n, u.T, steps_done, s);
}

hipError_t mz_launch_qtab_rehash(const MzQhash& from, const MzQhash& to, int T, int width,
                                 hipStream_t s) {
  const int64_t total = (int64_t)T * from.C;
  if (total <= 0) return hipSuccess;
  const int64_t want = (total + QT_T - 1) / QT_T;
  const dim3 grid((unsigned)(want < QH_MAX_BLOCKS ? want : QH_MAX_BLOCKS)), block(QT_T);
  if (width == 2)
    hipLaunchKernelGGL(k_qtab_rehash<2>, grid, block, 0, s, from, to, total);
  else
    hipLaunchKernelGGL(k_qtab_rehash<1>, grid, block, 0, s, from, to, total);
  return hipGetLastError();
}

hipError_t mz_launch_qtab_lookup(const MzQhash& h, int T, int width, const int32_t* tables,
                                 const int64_t* keys, int m, double* rows_out, int32_t* slots_out,
                                 hipStream_t s) {
  if (m <= 0) return hipSuccess;
  if (width == 2)
    hipLaunchKernelGGL(k_qtab_lookup<2>, qtab_grid(m), dim3(QT_T), 0, s, Hashed<2>{h}, T, tables,
                       keys, m, rows_out, slots_out);
  else
    hipLaunchKernelGGL(k_qtab_lookup<1>, qtab_grid(m), dim3(QT_T), 0, s, Hashed<1>{h}, T, tables,
                       keys, m, rows_out, slots_out);
  return hipGetLastError();
}
