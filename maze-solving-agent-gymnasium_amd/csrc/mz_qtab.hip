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
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mz_common.h"
#include "mz_learner.h"

namespace {

constexpr int QT_T = 256;  // threads per workgroup, one instance per lane

__device__ inline int qtab_coord(float v, int P) {  // a cell coordinate, never outside the pitch
  const int x = (int)v;
  return x < 0 ? 0 : (x >= P ? P - 1 : x);
}

// best-dir class from (br, bc): see the header comment
__device__ inline int qtab_dir(float brf, float bcf) {
  const int br = (int)brf, bc = (int)bcf;
  if (br == -1 || br > 1) return 1;
  if (br == 1 || br < -1) return 2;
  if (bc == -1 || bc > 1) return 3;
  if (bc == 1 || bc < -1) return 4;
  return 0;
}

__device__ inline int64_t qtab_index(const float* obs6, int i, int P) {
  const float2* o = reinterpret_cast<const float2*>(obs6 + (size_t)i * 6);  // 24-B rows: 8-B aligned
  const float2 a = o[0], g = o[1], b = o[2];
  const int64_t cell = (int64_t)qtab_coord(a.x, P) * P + qtab_coord(a.y, P);
  const int64_t goal = (int64_t)qtab_coord(g.x, P) * P + qtab_coord(g.y, P);
  return (cell * P * P + goal) * 5 + qtab_dir(b.x, b.y);
}

struct Row { double v[4]; };

__device__ inline Row qtab_load(const double* q, int64_t rows, int t, int64_t s) {
  const double2* p = reinterpret_cast<const double2*>(q + ((int64_t)t * rows + s) * 4);
  const double2 lo = p[0], hi = p[1];
  return Row{{lo.x, lo.y, hi.x, hi.y}};
}

__device__ inline double qtab_max(const Row& r) {  // np.max of the row
  double m = r.v[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) m = r.v[k] > m ? r.v[k] : m;
  return m;
}

__device__ inline int qtab_table(const int32_t* table_of, int i, int T) {
  const int t = table_of ? table_of[i] : i;
  return (unsigned)t < (unsigned)T ? t : -1;
}

__global__ __launch_bounds__(QT_T) void k_qtab_act(MzQtabAct a) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= a.n) return;
  const int t = (a.active && !a.active[i]) ? -1 : qtab_table(a.table_of, i, a.T);
  if (t < 0) {  // idle or no table: observe only (mz_step ignores a negative action)
    a.actions[i] = -1;
    a.sidx[i] = -1;
    return;
  }
  const int64_t s = qtab_index(a.obs6, i, a.P);
  const Row row = qtab_load(a.q, a.rows, t, s);
  const double x = __ddiv_rn(__dmul_rn(-1.0, (double)a.steps_done[t]), a.eps_decay[t]);
  const double ef = a.eps_final[t];
  const double eps = __dadd_rn(ef, __dmul_rn(__dsub_rn(a.eps_init[t], ef), exp(x)));
  uint32_t w[4];
  mz_philox(a.seed, MZ_QTAB_STREAM ^ ((uint64_t)(uint32_t)i << 32), a.counter, w);
  const double u = (double)(w[0] >> 8) * (1.0 / 16777216.0);
  int act;
  if (u < eps) {
    act = (int)(w[1] >> 30);
  } else {
    act = 0;
    double m = row.v[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
      if (row.v[k] > m) { m = row.v[k]; act = k; }
  }
  a.actions[i] = act;
  a.sidx[i] = s;
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

// What one instance's step contributes: the row / action it updates and lr * td.
struct Td {
  int t, act;
  int64_t s;
  double add, old;
};

__device__ inline bool qtab_td(const MzQtabUpd& u, int i, Td& o) {
  o.t = qtab_table(u.table_of, i, u.T);
  if (o.t < 0) return false;
  o.s = u.sidx[i];
  o.act = u.actions[i];
  if (o.s < 0 || o.s >= u.rows || (unsigned)o.act > 3u) return false;
  const int64_t s2 = qtab_index(u.obs6, i, u.P);
  const Row nxt = qtab_load(u.q, u.rows, o.t, s2);
  const Row cur = qtab_load(u.q, u.rows, o.t, o.s);
  const double future = u.terminated[i] ? 0.0 : qtab_max(nxt);
  const double q01 = (o.act & 1) ? cur.v[1] : cur.v[0], q23 = (o.act & 1) ? cur.v[3] : cur.v[2];
  o.old = (o.act & 2) ? q23 : q01;
  const double td = __dsub_rn(__dadd_rn(u.reward64[i], __dmul_rn(u.gamma[o.t], future)), o.old);
  o.add = __dmul_rn(u.lr[o.t], td);
  return true;
}

// independent tables (table_of NULL): nobody else touches instance i's table, gamma or counters
__global__ __launch_bounds__(QT_T) void k_qtab_update(MzQtabUpd u) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= u.n) return;
  Td d;
  if (!qtab_td(u, i, d)) return;
  u.q[((int64_t)d.t * u.rows + d.s) * 4 + d.act] = __dadd_rn(d.old, d.add);
  const double cum = __dadd_rn(u.cum[i], u.reward64[i]);
  const bool term = u.terminated[i] != 0;
  if (u.episode_end && (term || u.truncated[i])) {
    const double eta = u.eta[d.t];
    u.gamma[d.t] = __dadd_rn(u.gamma[d.t], cum > 0.0 ? eta : -eta);
    u.cum[i] = 0.0;
    u.episodes[d.t] += 1;
    u.wins[d.t] += term ? 1 : 0;
  } else {
    u.cum[i] = cum;
  }
}

// shared tables, pass 1: read-only on the table and on gamma
__global__ __launch_bounds__(QT_T) void k_qtab_td(MzQtabUpd u) {
  const int i = blockIdx.x * QT_T + threadIdx.x;
  if (i >= u.n) return;
  Td d;
  u.td[i] = qtab_td(u, i, d) ? d.add : 0.0;
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
  const double cum = __dadd_rn(u.cum[i], u.reward64[i]);
  const bool term = u.terminated[i] != 0;
  if (u.episode_end && (term || u.truncated[i])) {
    const double eta = u.eta[t];
    unsafeAtomicAdd(u.gamma + t, cum > 0.0 ? eta : -eta);
    u.cum[i] = 0.0;
    atomicAdd(reinterpret_cast<unsigned long long*>(u.episodes + t), 1ull);
    if (term) atomicAdd(reinterpret_cast<unsigned long long*>(u.wins + t), 1ull);
  } else {
    u.cum[i] = cum;
  }
}

}  // namespace

hipError_t mz_launch_qtab_act(const MzQtabAct& a, long long* steps_done, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const int blocks = (a.n + QT_T - 1) / QT_T;
  hipLaunchKernelGGL(k_qtab_act, dim3(blocks), dim3(QT_T), 0, s, a);
  hipLaunchKernelGGL(k_qtab_advance, dim3(blocks), dim3(QT_T), 0, s, a.table_of, a.active,
                     a.n, a.T, steps_done);
  return hipGetLastError();
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
