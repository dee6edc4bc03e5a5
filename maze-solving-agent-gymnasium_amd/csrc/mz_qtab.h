// mz_qtab.h — device helpers of the vectorised tabular learners (mz_qtab.hip): Q-learning and double
// Q-learning on dense or hashed tables. The state index, the epsilon expression, the action choice,
// the TD expressions and the episode end are written once, here, so that the float64 operation order
// (__dmul_rn / __dadd_rn ...) cannot drift between the storages and the rules. What varies is two
// small types the kernels are templates over:
//   a storage (Dense<W> / Hashed<W>, W rows of 4 f64 per state: 1 for Q, 2 = A and B for double Q)
//     says where state s of table t is, what rows are there, and how a value is stored or added;
//   a rule (RuleQ / RuleDQ) yields the td from the fetched rows, says which row the write goes to
//     and whether took / which are written.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mz_common.h"
#include "mz_learner.h"
#include "mz_qhash.h"

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

constexpr Row ZERO_ROW{{0.0, 0.0, 0.0, 0.0}};

// ---- storages ------------------------------------------------------------------------------------
// A state holds W rows: Q's row, or double Q's A row (0) and B row (1), side by side.
// find(t, s) locates state s of table t; row(l, k) reads row k there (an absent key reads as zeros);
// store writes element e (row * 4 + action) of the located state by plain loads and stores, for a
// lane that owns table t; add is one f64 atomic add of *v into element e of state s, for lanes that
// share tables, and reads no row (*v, the lr * td of pass 1, is fetched once the element is there,
// not ahead of the probe). A state is W * 32-B aligned.
template <int W>
struct Dense {  // q [T][rows][W][4]
  double* q;
  int64_t rows;
  struct Loc { int64_t at; };  // of the state's first element
  __device__ Loc find(int t, int64_t s) const { return Loc{((int64_t)t * rows + s) * (4 * W)}; }
  __device__ Row row(const Loc& l, int k) const { return qtab_row_at(q + l.at + 4 * k); }
  __device__ void store(const Loc& l, int, int64_t, int e, double v) const { q[l.at + e] = v; }
  __device__ void add(int t, int64_t s, int e, const double* v) const {
    unsafeAtomicAdd(q + find(t, s).at + e, *v);
  }
};

template <int W>
struct Hashed {  // h.keys [T][C], h.vals [T][C][W][4]: see mz_qtab.hip
  MzQhash h;
  struct Loc { int64_t base; uint32_t slot; int state; };  // the probe's outcome, kept for store
  __device__ Loc find(int t, int64_t s) const {
    Loc l{(int64_t)t * h.C, 0u, QH_FULL};
    l.state = qhash_probe(h.keys + l.base, h.C, h.shift, (int32_t)s, l.slot);
    return l;
  }
  __device__ Row row(const Loc& l, int k) const {
    if (l.state != QH_FOUND) return ZERO_ROW;
    return qtab_row_at(h.vals + (l.base + l.slot) * (4 * W) + 4 * k);
  }
  // the key is inserted on every write, also of a zero value; a full table drops and counts it
  __device__ void store(const Loc& l, int t, int64_t s, int e, double v) const {
    if (l.state == QH_FULL) {
      h.overflow[t] += 1;
      return;
    }
    const int64_t at = l.base + l.slot;
    if (l.state == QH_EMPTY) {
      h.keys[at] = (int32_t)s;
      h.load[t] += 1;
    }
    h.vals[at * (4 * W) + e] = v;
  }
  // find or insert under concurrent inserts (qhash_claim), then the add; a full table counts the drop
  __device__ void add(int t, int64_t s, int e, const double* v) const {
    const int64_t base = (int64_t)t * h.C;
    uint32_t slot;
    bool fresh;
    if (qhash_claim(h.keys + base, h.C, h.shift, (int32_t)s, slot, fresh)) {
      if (fresh) atomicAdd(h.load + t, 1);
      unsafeAtomicAdd(h.vals + (base + slot) * (4 * W) + e, *v);
    } else {
      atomicAdd(reinterpret_cast<unsigned long long*>(h.overflow + t), 1ull);
    }
  }
};

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

// What one instance's update contributes: the element it updates and lr * td.
struct Td {
  int t, act, which;  // which: the row written, 0 = Q / Q_A, 1 = Q_B
  int64_t s;
  double add, old;
};

// The guard of every update stage: instance i's table, the row it acted from and its action. False:
// the instance sits this update out (no table, no act() before it, an action that is none).
__device__ inline bool qtab_who(const MzQtabUpd& u, int i, int& t, int64_t& s, int& act) {
  t = qtab_table(u.table_of, i, u.T);
  if (t < 0) return false;
  s = u.sidx[i];
  act = u.actions[i];
  return s >= 0 && s < u.rows && (unsigned)act <= 3u;
}

// QAgent.update's td. The storage is asked for s' first and for s last; `at` is where s is, for the
// store that follows (one probe each on hashed tables).
template <class S>
__device__ inline bool qtab_td(const MzQtabUpd& u, int i, Td& o, const S& st,
                               typename S::Loc& at) {
  if (!qtab_who(u, i, o.t, o.s, o.act)) return false;
  o.which = 0;
  const int64_t s2 = qtab_index(u.obs6, i, u.P);
  const Row nxt = st.row(st.find(o.t, s2), 0);
  at = st.find(o.t, o.s);
  const Row cur = st.row(at, 0);
  const double future = u.terminated[i] ? 0.0 : qtab_max(nxt);
  o.old = qtab_pick(cur, o.act);
  const double td = __dsub_rn(__dadd_rn(u.reward64[i], __dmul_rn(u.gamma[o.t], future)), o.old);
  o.add = __dmul_rn(u.lr[o.t], td);
  return true;
}

// DQAgent.update's td: the coin, the inner get_action on Q_A[s'], the value of the other table. Both
// rows of s' and of s are fetched, in that order (one 64-B segment each).
template <class S>
__device__ inline bool dqtab_td(const MzDqtabUpd& d, int i, Td& o, const S& st,
                                typename S::Loc& at) {
  const MzQtabUpd& u = d.u;
  if (!qtab_who(u, i, o.t, o.s, o.act)) return false;
  int best = d.next_action ? d.next_action[i] : 0;
  if ((unsigned)best > 3u) return false;
  const int64_t s2 = qtab_index(u.obs6, i, u.P);
  const typename S::Loc at2 = st.find(o.t, s2);
  const Row nxt_a = st.row(at2, 0), nxt_b = st.row(at2, 1);
  at = st.find(o.t, o.s);
  const Row cur_a = st.row(at, 0), cur_b = st.row(at, 1);
  uint32_t w[4];
  mz_philox(d.seed, MZ_DQTAB_STREAM ^ ((uint64_t)(uint32_t)i << 32), d.ucounter, w);
  const bool to_a = d.coin ? d.coin[i] == 0 : (double)(w[0] >> 8) * (1.0 / 16777216.0) < 0.5;
  if (!d.next_action) {  // the inner get_action on Q_A[s']
    const double eps =
        qtab_eps(d.steps_done[o.t], d.eps_init[o.t], d.eps_final[o.t], d.eps_decay[o.t]);
    const double u2 = (double)(w[1] >> 8) * (1.0 / 16777216.0);
    best = u2 < eps ? (int)(w[2] >> 30) : qtab_argmax(nxt_a);
  }
  o.which = to_a ? 0 : 1;
  const double other = to_a ? qtab_pick(nxt_b, best) : qtab_pick(nxt_a, best);
  o.old = to_a ? qtab_pick(cur_a, o.act) : qtab_pick(cur_b, o.act);
  const double td = __dsub_rn(__dadd_rn(u.reward64[i], __dmul_rn(u.gamma[o.t], other)), o.old);
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

// ---- rules ---------------------------------------------------------------------------------------
// Args: what the update kernels take. td: the rule's td from the storage. took / which: what an
// update leaves for the stages behind it — Q leaves nothing and every lane applies into row 0;
// double Q writes took[i] (the advance that follows counts the inner get_actions by it) and, between
// the two shared-table passes, the row it chose.
struct RuleQ {
  using Args = MzQtabUpd;
  static const Args& of(const MzDqtabUpd& d) { return d.u; }  // (host) the launcher's arguments
  static __device__ const MzQtabUpd& upd(const Args& a) { return a; }
  template <class S>
  static __device__ bool td(const Args& a, int i, Td& o, const S& st, typename S::Loc& at) {
    return qtab_td(a, i, o, st, at);
  }
  static __device__ void set_took(const Args&, int, bool) {}
  static __device__ void set_which(const Args&, int, int) {}
  static __device__ bool took(const Args&, int) { return true; }
  static __device__ int which(const Args&, int) { return 0; }
};

struct RuleDQ {
  using Args = MzDqtabUpd;
  static const Args& of(const MzDqtabUpd& d) { return d; }
  static __device__ const MzQtabUpd& upd(const Args& a) { return a.u; }
  template <class S>
  static __device__ bool td(const Args& a, int i, Td& o, const S& st, typename S::Loc& at) {
    return dqtab_td(a, i, o, st, at);
  }
  static __device__ void set_took(const Args& a, int i, bool ok) { a.took[i] = ok; }
  static __device__ void set_which(const Args& a, int i, int w) { a.which[i] = (uint8_t)w; }
  static __device__ bool took(const Args& a, int i) { return a.took[i] != 0; }
  static __device__ int which(const Args& a, int i) { return a.which[i] ? 1 : 0; }
};

}  // namespace
