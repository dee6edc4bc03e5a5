// mz_qtab.hip — config 1 vectorised: a population of tabular Q-learners whose tables live in HBM.
//
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
// The index, the epsilon / action choice, the TD expression and the episode end live in mz_qtab.h,
// shared with the hashed storage (mz_qhash.hip); this file supplies the dense row fetch and store.
#include "mz_qtab.h"

namespace {

__device__ inline Row qtab_load(const double* q, int64_t rows, int t, int64_t s) {
  return qtab_row_at(q + ((int64_t)t * rows + s) * 4);
}

__global__ __launch_bounds__(QT_T) void k_qtab_act(MzQtabAct a) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= a.n) return;
  const int t = qtab_act_table(a, i);
  if (t < 0) return;  // idle or no table: observe only
  const int64_t s = qtab_index(a.obs6, i, a.P);
  qtab_choose(a, i, t, s, qtab_load(a.q, a.rows, t, s));
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

struct DenseFetch {
  const double* q;
  int64_t rows;
  __device__ Row operator()(int t, int64_t s) const { return qtab_load(q, rows, t, s); }
};

// independent tables (table_of NULL): nobody else touches instance i's table, gamma or counters
__global__ __launch_bounds__(QT_T) void k_qtab_update(MzQtabUpd u) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= u.n) return;
  Td d;
  if (!qtab_td(u, i, d, DenseFetch{u.q, u.rows})) return;
  u.q[((int64_t)d.t * u.rows + d.s) * 4 + d.act] = __dadd_rn(d.old, d.add);
  qtab_end_plain(u, i, d.t);
}

// shared tables, pass 1: read-only on the table and on gamma
__global__ __launch_bounds__(QT_T) void k_qtab_td(MzQtabUpd u) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= u.n) return;
  Td d;
  u.td[i] = qtab_td(u, i, d, DenseFetch{u.q, u.rows}) ? d.add : 0.0;
}

// shared tables, pass 2: one f64 atomic add per instance, then the episode end
__global__ __launch_bounds__(QT_T) void k_qtab_apply(MzQtabUpd u) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= u.n) return;
  const int t = qtab_table(u.table_of, i, u.T);
  if (t < 0) return;
  const int64_t s = u.sidx[i];
  const int act = u.actions[i];
  if (s < 0 || s >= u.rows || (unsigned)act > 3u) return;
  unsafeAtomicAdd(u.q + ((int64_t)t * u.rows + s) * 4 + act, u.td[i]);
  qtab_end_atomic(u, i, t);
}

}  // namespace

hipError_t mz_launch_qtab_advance(const int32_t* table_of, const uint8_t* active, int n, int T,
                                  long long* steps_done, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_qtab_advance, dim3((n + QT_T - 1) / QT_T), dim3(QT_T), 0, s, table_of,
                     active, n, T, steps_done);
  return hipGetLastError();
}

hipError_t mz_launch_qtab_act(const MzQtabAct& a, long long* steps_done, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const int blocks = (a.n + QT_T - 1) / QT_T;
  hipLaunchKernelGGL(k_qtab_act, dim3(blocks), dim3(QT_T), 0, s, a);
  return mz_launch_qtab_advance(a.table_of, a.active, a.n, a.T, steps_done, s);
}

hipError_t mz_launch_qtab_update(const MzQtabUpd& u, hipStream_t s) {
  if (u.n <= 0) return hipSuccess;
  const int blocks = (u.n + QT_T - 1) / QT_T;
  if (!u.table_of) {
    hipLaunchKernelGGL(k_qtab_update, dim3(blocks), dim3(QT_T), 0, s, u);
  } else {
    hipLaunchKernelGGL(k_qtab_td, dim3(blocks), dim3(QT_T), 0, s, u);
    hipLaunchKernelGGL(k_qtab_apply, dim3(blocks), dim3(QT_T), 0, s, u);
  }
  return hipGetLastError();
}
