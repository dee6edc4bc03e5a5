// mz_qtab.h — device helpers shared by the vectorised tabular learners: mz_qtab.hip (dense tables),
// mz_qhash.hip (hashed tables) and mz_dqtab.hip (double Q-learning on either). The state index, the epsilon
// expression, the action choice, the TD expression and the episode end are written once, here, so
// that the float64 operation order (__dmul_rn / __dadd_rn ...) cannot drift between the storages:
// a storage only supplies how a row is fetched and where the new value goes.
#pragma once
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

// best-dir class from (br, bc): see the header comment of mz_qtab.hip
__device__ inline int qtab_dir(float brf, float bcf) {
  const int br = (int)brf, bc = (int)bcf;
  if (br == -1 || br > 1) return 1;
  if (br == 1 || br < -1) return 2;
  if (bc == -1 || bc > 1) return 3;
  if (bc == 1 || bc < -1) return 4;
  return 0;
}

__device__ inline int64_t qtab_index(const float* obs6, int i, int P) {
  // 24-B rows: 8-B aligned
  const float2* o = reinterpret_cast<const float2*>(obs6 + (size_t)i * 6);
  const float2 a = o[0], g = o[1], b = o[2];
  const int64_t cell = (int64_t)qtab_coord(a.x, P) * P + qtab_coord(a.y, P);
  const int64_t goal = (int64_t)qtab_coord(g.x, P) * P + qtab_coord(g.y, P);
  return (cell * P * P + goal) * 5 + qtab_dir(b.x, b.y);
}

struct Row { double v[4]; };

__device__ inline Row qtab_row_at(const double* p4) {  // 4 f64 at a 16-B aligned address
  const double2* p = reinterpret_cast<const double2*>(p4);
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

// The acting instance's table, or -1 (idle: the action and the row index are written as -1; mz_step
// ignores a negative action).
__device__ inline int qtab_act_table(const MzQtabAct& a, int i) {
  const int t = (a.active && !a.active[i]) ? -1 : qtab_table(a.table_of, i, a.T);
  if (t < 0) {
    a.actions[i] = -1;
    a.sidx[i] = -1;
  }
  return t;
}

// eps = final + (init - final) * exp(-1.0 * steps_done / decay), the reference's expression order
__device__ inline double qtab_eps(long long steps_done, double init, double ef, double decay) {
  const double x = __ddiv_rn(__dmul_rn(-1.0, (double)steps_done), decay);
  return __dadd_rn(ef, __dmul_rn(__dsub_rn(init, ef), exp(x)));
}

__device__ inline int qtab_argmax(const Row& row) {  // np.argmax: the row's first maximum
  int act = 0;
  double m = row.v[0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (row.v[k] > m) { m = row.v[k]; act = k; }
  return act;
}

__device__ inline double qtab_pick(const Row& r, int k) {  // r.v[k] by selects (no scratch)
  const double q01 = (k & 1) ? r.v[1] : r.v[0], q23 = (k & 1) ? r.v[3] : r.v[2];
  return (k & 2) ? q23 : q01;
}

// get_action from the fetched row of state s: eps, one Philox draw, the row's first maximum.
__device__ inline void qtab_choose(const MzQtabAct& a, int i, int t, int64_t s, const Row& row) {
  const double eps = qtab_eps(a.steps_done[t], a.eps_init[t], a.eps_final[t], a.eps_decay[t]);
  uint32_t w[4];
  mz_philox(a.seed, MZ_QTAB_STREAM ^ ((uint64_t)(uint32_t)i << 32), a.counter, w);
  const double u = (double)(w[0] >> 8) * (1.0 / 16777216.0);
  a.actions[i] = u < eps ? (int)(w[1] >> 30) : qtab_argmax(row);
  a.sidx[i] = s;
}

// What one instance's step contributes: the row / action it updates and lr * td.
struct Td {
  int t, act;
  int64_t s;
  double add, old;
};

// fetch(t, s) -> Row is the storage's read of row s of table t. It is called for s' first and for
// s last (a hashed fetch leaves the probe of s behind for the store that follows).
template <class Fetch>
__device__ inline bool qtab_td(const MzQtabUpd& u, int i, Td& o, Fetch&& fetch) {
  o.t = qtab_table(u.table_of, i, u.T);
  if (o.t < 0) return false;
  o.s = u.sidx[i];
  o.act = u.actions[i];
  if (o.s < 0 || o.s >= u.rows || (unsigned)o.act > 3u) return false;
  const int64_t s2 = qtab_index(u.obs6, i, u.P);
  const Row nxt = fetch(o.t, s2);
  const Row cur = fetch(o.t, o.s);
  const double future = u.terminated[i] ? 0.0 : qtab_max(nxt);
  o.old = qtab_pick(cur, o.act);
  const double td = __dsub_rn(__dadd_rn(u.reward64[i], __dmul_rn(u.gamma[o.t], future)), o.old);
  o.add = __dmul_rn(u.lr[o.t], td);
  return true;
}

// The episode end of instance i on table t. Plain: nobody else touches t's gamma or counters.
__device__ inline void qtab_end_plain(const MzQtabUpd& u, int i, int t) {
  const double cum = __dadd_rn(u.cum[i], u.reward64[i]);
  const bool term = u.terminated[i] != 0;
  if (u.episode_end && (term || u.truncated[i])) {
    const double eta = u.eta[t];
    u.gamma[t] = __dadd_rn(u.gamma[t], cum > 0.0 ? eta : -eta);
    u.cum[i] = 0.0;
    u.episodes[t] += 1;
    u.wins[t] += term ? 1 : 0;
  } else {
    u.cum[i] = cum;
  }
}

// Shared tables: gamma and the counters take atomic adds.
__device__ inline void qtab_end_atomic(const MzQtabUpd& u, int i, int t) {
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
