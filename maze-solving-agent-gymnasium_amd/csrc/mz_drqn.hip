// mz_drqn.hip — the recurrent DQN (agents/lstm_dqn_agent.py: nn.LSTMCell(6, 32) + nn.Linear(32, 4)
// over obs6) on the device: the acting step with its per-instance (h, c), the episode replay
// memory, and the sequence forward / TD target / back-propagation through time of an update.
//
// The net (5,252 parameters, torch's layouts and gate order i, f, g, o):
//   z = (bias_ih + bias_hh) + W_ih x + W_hh h      [128]
//   c' = sigmoid(z_f) c + sigmoid(z_i) tanh(z_g),  h' = sigmoid(z_o) tanh(c'),  q = fc_b + fc_w h'
// ACCUMULATION ORDER, the same in every kernel here: a gate pre-activation starts from the f32 sum
// bias_ih + bias_hh, then takes the 6 input terms k = 0..5, then the 32 recurrent terms k = 0..31,
// one fmaf each; a q value starts from fc_b and takes the 32 terms k = 0..31, one fmaf each.
// sigmoid(z) = 1 / (1 + expf(-z)); tanh is tanhf.
//
// Per vector step (trainers/drqn_trainer.py VectorRecurrentDQNTrainer):
//   k_drqn_act    four lanes per instance, eight units each. The parameters are staged in LDS once
//                 per workgroup; the old h is held in registers, c streams through; both live
//                 in HBM as [32][B] so a wave's loads and stores coalesce. One Philox
//                 draw per instance decides explore / greedy and the uniform action. Records
//                 (x_t, a_t) at t[i]; zero state where t[i] == 0. L == 0 is the evaluation mode:
//                 nothing is recorded and every instance's state advances.
//   (mz_step, k_ppo_scan)   the reward record, t[i] += 1, the finished episodes' list
//   k_drqn_store  one workgroup per finished episode: x_n into the record, the episode into the
//                 ring slot (head + k) mod capacity; k_drqn_ring advances head and count.
// Per update:
//   k_drqn_sample    one wave: E distinct slots of the filled ring (Floyd's subset sampling), the
//                    batch directory (slot, length, row offset, totals).
//   k_drqn_seq_fwd   one wave per episode. Lane l = (unit u = l & 31, half = l >> 5) owns gate rows
//                    (i_u, f_u) or (g_u, o_u): its 2 x 38 weights stay in registers for the whole
//                    episode, h goes round through LDS. Target mode writes max_a Q'_t; source mode
//                    stashes (i, f, g, o, c, h) per step (768 B a row), and writes Q_t[a_t], y_t,
//                    the scaled residual 2 (Q_t[a_t] - y_t) / sum n and the episode's sum of
//                    squared residuals (float64, time order).
//   k_drqn_seq_bwd   one wave per episode, same lane layout: BPTT from the stash; the weight
//                    gradients accumulate in registers over the time loop and are written once,
//                    as the episode's partial in the flat parameter order.
//   k_drqn_reduce    per parameter the partials summed over the episodes in index order (float64,
//                    rounded once) into the net's gradient segments; the loss (float64, episode
//                    order). No float atomics anywhere: two runs give the same bits.
// Replay windows (window = T, burn_in = K; off by default):
//   k_drqn_snapshot    a launch of its own before k_drqn_act (whose code and bits stay as they
//                      are): the state an instance acts from at t = j T, j >= 1, into its record.
//   k_drqn_snap_store  before k_drqn_store: the finished episodes' snapshots into the ring slot
//                      k_drqn_store is about to give them.
//   k_drqn_win_sample  k_drqn_sample's body for the slots, then one window per episode and the
//                      window directory; a window owns m + 2 rows (entry state, m steps, guard),
//                      so the row buffers hold E (T + 2) rows whatever L and K are.
//   k_drqn_win_fwd / k_drqn_win_bwd   the sequence kernels' time loops (drqn_unroll_fwd / _bwd: a
//                      whole episode is the window b = 0, k = 0, m = n from zero state) over steps
//                      b .. of the episode from the stored state; the burn-in steps only advance the
//                      state, BPTT covers the m training steps. k_drqn_reduce sums the per-window
//                      partials.
// Prioritized windows (priority_alpha; off by default): every window (slot, j) carries an integer
// mass, so every sum is exact and the sampler equals a host model bit for bit.
//   k_drqn_prio_store   before k_drqn_store: the finished episodes' windows enter at prio_max.
//   k_drqn_prio_sample  in k_drqn_win_sample's place, one workgroup per learner: windows in
//                       proportion to their mass (stratified, with replacement), the same
//                       directory, and the importance weights.
//   k_drqn_prio_update  between k_drqn_win_fwd (source) and k_drqn_win_bwd, one workgroup per
//                       learner: the sampled windows' new masses from the forward's residuals,
//                       the slots' sums, and d and ep_loss scaled by the weights. The forward
//                       and backward kernels are not touched.
// Double-Q targets and n-step returns (double_q, n_step; off by default, and then none of these is
// launched): y is formed in a launch of its own between the source forward and the priority update.
//   k_drqn_seq_fwd_q / k_drqn_win_fwd_q   the forwards' second form (drqn_unroll_fwd<FWD_Q4 /
//                       FWD_SEL>): the target net writes all four Q'_t of rows row .. row + m, the
//                       source net its stash, Q_t[a_t] and the first argmax of its own Q_t, one
//                       step further than the old source mode.
//   k_drqn_seq_ret / k_drqn_win_ret   one wave per span: the n-step return of every training
//                       step (float32 fmaf chain, cut at the span's end), bootstrapped from the
//                       selected or the largest Q', into y; d and ep_loss as the old source mode.
// Populations (trainers/drqn_population.py VectorRecurrentDQNPopulation): P independent learners
// over B = P b instances, learner p owning instances [p b, (p + 1) b), flat [P][5252] parameters.
// Every kernel above but k_drqn_snapshot (which serves B = P b as it is) moves its single-learner
// argument struct to learner p's rows (parameters, ring, directory, row buffers, eps / seed /
// gamma / update count / burn-in) and runs the __device__ body on it; the single learner is the
// launch with P = 1, b = B and null per-learner arrays, where every row offset is zero and the
// struct's by-value fields stand. Grids: act P x ceil(b / 16) workgroups (none straddles two
// learners); store and snapshot store (., P) workgroups, learner p's run of the finished list
// found by two binary searches; the samplers P waves; the sequence and window kernels P E waves;
// reduce and the target sync k_drqn_pop_sync (21, P). Waves of a learner that is not due exit at
// once.
// Replay windows in a population: T is shared, the burn-in K_p and stored / zero state are per
// learner; k_drqn_reduce reads the m row of learner p's directory block. A K_p that breaks the
// rule (negative, no multiple of T, above K_max) lives on the device and cannot be refused: that
// learner's view gets K = -1, which no window passes, so its batch has no window, nothing of its
// row buffers is written and its partials are zero.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mz_common.h"
#include "mz_learner.h"

namespace {

constexpr int WAVE = 64;
constexpr int H = MZ_DRQN_HIDDEN;  // 32
constexpr int G4 = 4 * H;          // 128 gate rows
constexpr int NX = 6;
constexpr int ACT_T = 64;          // k_drqn_act threads: one wave, so the workgroups spread over the CUs
constexpr int ROW = MZ_DRQN_ROW_WORDS;  // 8 words per replay row: x[6], action, reward
constexpr int STASH = MZ_DRQN_STASH;    // 192 floats per stashed step
// offsets into the flat parameter order
constexpr int P_WIH = 0, P_WHH = P_WIH + G4 * NX, P_BIH = P_WHH + G4 * H, P_BHH = P_BIH + G4,
              P_FCW = P_BHH + G4, P_FCB = P_FCW + 4 * H;
static_assert(P_FCB + 4 == MZ_DRQN_PARAMS, "parameter count");
// mz_drqn_flat_net (mz_learner.h) splits a population's flat row at these offsets
static_assert(P_WHH == 768 && P_BIH == 768 + 4096 && P_BHH == P_BIH + 128 && P_FCW == P_BHH + 128 &&
              P_FCB == P_FCW + 128, "flat row offsets");

__device__ inline float sigmoidf_(float z) { return 1.0f / (1.0f + expf(-z)); }

// LDS image of the parameters for k_drqn_act: per gate row 40 floats (bias, 6 x, pad, 32 h) so a
// row starts 16-B aligned; then fc (4 x 32) and fc_b
constexpr int AROW = 40;
constexpr int A_FC = G4 * AROW, A_FCB = A_FC + 4 * H, A_TOT = A_FCB + 4;
#ifndef MZ_DRQN_ACT_PARTS
#define MZ_DRQN_ACT_PARTS 4  // threads per instance (1, 2 or 4; profiles/exp_lstm_dqn_probe.py)
#endif
constexpr int PARTS = MZ_DRQN_ACT_PARTS;
constexpr int IPB = ACT_T / PARTS;  // instances per workgroup
static_assert(PARTS == 1 || PARTS == 2 || PARTS == 4, "threads per instance");

// Thread (j = tid % IPB, part = tid / IPB) of instance i = block * IPB + j computes the units
// u = part, part + PARTS, ...: the parts of one instance sit IPB lanes apart, so a wave's loads of
// h / c ([32][B]) stay coalesced, and their weight rows sit AROW = 40 floats apart in LDS, which
// puts the (up to 4) distinct 16-B addresses of a wave's ds_read_b128 on different banks. Every
// thread holds the instance's whole old h in registers. The new h goes round through LDS for the
// head: part a computes q[a] (a + PARTS, ...) in the fixed order, part 0 draws and records.
// blk: the workgroup's index among the workgroups of q's B instances; ld: the pitch of h / c (the
// launch's whole instance count: q may be one learner's block of a population's arrays). The Philox
// draw is keyed by the instance's index within q.
__device__ __forceinline__ void drqn_act_body(const MzDrqnAct& q, const int blk, const size_t B) {
  __shared__ __attribute__((aligned(16))) float w[A_TOT];
  __shared__ float hq[IPB][H + 1];
  __shared__ float qs[IPB][4];
  for (int e = threadIdx.x; e < G4; e += ACT_T) {
    float* d = w + e * AROW;
    d[0] = q.p.b_ih[e] + q.p.b_hh[e];
    for (int k = 0; k < NX; ++k) d[1 + k] = q.p.w_ih[e * NX + k];
    for (int k = 0; k < H; ++k) d[8 + k] = q.p.w_hh[e * H + k];
    d[7] = 0.0f;
  }
  for (int e = threadIdx.x; e < 4 * H; e += ACT_T) w[A_FC + e] = q.p.fc_w[e];
  if (threadIdx.x < 4) w[A_FCB + threadIdx.x] = q.p.fc_b[threadIdx.x];
  __syncthreads();
  const int j = threadIdx.x % IPB, part = threadIdx.x / IPB;
  const int i = blk * IPB + j;
  const bool live = i < q.B;
  const int ii = live ? i : q.B - 1;  // a tail thread shadows the last instance and writes nothing
  const int t = q.t[ii];
  const bool eval = q.L == 0;
  const bool rec = live && t >= 0 && t < q.L;
  const bool adv = live && (rec || eval);  // the state advances
  const bool zero = t == 0;
  float x[NX], h[H];
#pragma unroll
  for (int k = 0; k < NX; ++k) x[k] = q.obs6[(size_t)ii * NX + k];
#pragma unroll
  for (int k = 0; k < H; ++k) h[k] = zero ? 0.0f : q.h[k * B + ii];
  // every part has read the old h before any part stores a new one (h_out may alias h)
  __syncthreads();
  for (int u = part; u < H; u += PARTS) {
    float z[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4* r = reinterpret_cast<const float4*>(w + (g * H + u) * AROW);
      const float4 r0 = r[0], r1 = r[1];
      float acc = r0.x;
      acc = fmaf(r0.y, x[0], acc);
      acc = fmaf(r0.z, x[1], acc);
      acc = fmaf(r0.w, x[2], acc);
      acc = fmaf(r1.x, x[3], acc);
      acc = fmaf(r1.y, x[4], acc);
      acc = fmaf(r1.z, x[5], acc);
#pragma unroll
      for (int k4 = 0; k4 < H / 4; ++k4) {
        const float4 v = r[2 + k4];
        acc = fmaf(v.x, h[4 * k4 + 0], acc);
        acc = fmaf(v.y, h[4 * k4 + 1], acc);
        acc = fmaf(v.z, h[4 * k4 + 2], acc);
        acc = fmaf(v.w, h[4 * k4 + 3], acc);
      }
      z[g] = acc;
    }
    const float c0 = zero ? 0.0f : q.c[u * B + ii];
    const float c1 = sigmoidf_(z[1]) * c0 + sigmoidf_(z[0]) * tanhf(z[2]);
    const float h1 = sigmoidf_(z[3]) * tanhf(c1);
    if (adv) {
      q.c_out[u * B + i] = c1;
      q.h_out[u * B + i] = h1;
    }
    hq[j][u] = h1;
  }
  __syncthreads();
  for (int a = part; a < 4; a += PARTS) {
    float acc = w[A_FCB + a];
#pragma unroll
    for (int k = 0; k < H; ++k) acc = fmaf(w[A_FC + a * H + k], hq[j][k], acc);
    qs[j][a] = acc;
  }
  __syncthreads();
  if (part != 0 || !live) return;
  const float qv[4] = {qs[j][0], qs[j][1], qs[j][2], qs[j][3]};
  // greedy: the first maximum (torch.max's index); a NaN row acts 0
  int a = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (qv[k] > qv[a]) a = k;
  uint32_t r[4];
  mz_philox(q.seed, MZ_DRQN_STREAM ^ ((uint64_t)(uint32_t)i << 32), q.counter, r);
  const float uni = (float)(r[0] >> 8) * (1.0f / 16777216.0f);  // [0, 1), 24 bits
  if (uni < q.eps) a = (int)(((uint64_t)r[1] * (uint64_t)q.explore) >> 32);
  if (rec) {
    float* dst = q.rec_x + ((size_t)i * (q.L + 1) + t) * NX;
#pragma unroll
    for (int k = 0; k < NX; ++k) dst[k] = x[k];
    q.rec_a[(size_t)i * q.L + t] = a;
  }
  q.act_out[i] = a;
  if (q.q_out) {
#pragma unroll
    for (int k = 0; k < 4; ++k) q.q_out[(size_t)i * 4 + k] = qv[k];
  }
}

// learner p's view of a population's flat [P][5252] parameters
__device__ __forceinline__ MzDrqnNet drqn_net_row(const MzDrqnNet& n, const int p) {
  const size_t o = (size_t)p * MZ_DRQN_PARAMS;
  return MzDrqnNet{n.w_ih + o, n.w_hh + o, n.b_ih + o, n.b_hh + o, n.fc_w + o, n.fc_b + o};
}

// The acting step: workgroup (p, blk) runs the body on learner p's block of b instances with its
// own parameters, eps and seed, so no workgroup straddles two learners (the tail workgroup of a
// learner is partly idle).
__global__ __launch_bounds__(ACT_T) void k_drqn_act(MzDrqnPopAct q) {
  const int bpl = (q.b + IPB - 1) / IPB;
  const int p = blockIdx.x / bpl;
  const size_t i0 = (size_t)p * q.b;
  MzDrqnAct a = q.a;
  a.p = drqn_net_row(q.a.p, p);
  a.B = q.b;
  if (q.eps) a.eps = q.eps[p];
  if (q.seed) a.seed = q.seed[p];
  a.obs6 += i0 * NX;
  a.t += i0;
  a.h += i0;
  a.c += i0;
  a.h_out += i0;
  a.c_out += i0;
  if (a.L > 0) {
    a.rec_x += i0 * (a.L + 1) * NX;
    a.rec_a += i0 * a.L;
  }
  a.act_out += i0;
  if (a.q_out) a.q_out += i0 * 4;
  drqn_act_body(a, blockIdx.x % bpl, (size_t)q.a.B);
}

// ---- replay memory ---------------------------------------------------------------------------
// the listed episodes fin_id / fin_len [0, nfin) into q's ring, episode k into slot (head + k) mod
// capacity; workgroup blk of nblk takes every nblk-th
__device__ __forceinline__ void drqn_store_body(const MzDrqnStore& q, const int32_t* fin_id,
                                                const int32_t* fin_len, const int nfin,
                                                const int blk, const int nblk) {
  const int64_t head = q.ring[0];
  // more finished episodes than slots: the last `capacity` stay (a deque's maxlen)
  const int first = nfin > q.cap ? nfin - (int)q.cap : 0;
  for (int k = first + blk; k < nfin; k += nblk) {
    const int i = fin_id[k], n = fin_len[k];
    if (i < 0 || i >= q.B || n < 1 || n > q.L || head < 0 || head >= q.cap) continue;
    const int64_t slot = (head + k) % q.cap;
    float* rx = q.rec_x + (size_t)i * (q.L + 1) * NX;
    if (threadIdx.x < NX) rx[(size_t)n * NX + threadIdx.x] = q.obs6[(size_t)i * NX + threadIdx.x];
    __syncthreads();
    uint32_t* dst = q.mem + (size_t)slot * (q.L + 1) * ROW;
    const int32_t* ra = q.rec_a + (size_t)i * q.L;
    const double* rr = q.rec_r + (size_t)i * q.L;
    for (int e = threadIdx.x; e < (n + 1) * ROW; e += blockDim.x) {
      const int t = e / ROW, j = e % ROW;
      uint32_t v = 0;
      if (j < NX) v = __float_as_uint(rx[(size_t)t * NX + j]);
      else if (t < n) v = j == NX ? (uint32_t)ra[t] : __float_as_uint((float)rr[t]);
      dst[e] = v;
    }
    if (threadIdx.x == 0) {
      q.mem_len[slot] = n;
      q.mem_term[slot] = q.term[i] != 0 ? 1 : 0;
    }
    __syncthreads();
  }
}

__device__ __forceinline__ void drqn_ring_advance(int64_t* ring, const int64_t nfin,
                                                  const int64_t cap) {
  const int64_t head = ring[0], count = ring[1];
  if (head < 0 || head >= cap) return;
  ring[0] = (head + nfin) % cap;
  ring[1] = count + nfin < cap ? count + nfin : cap;
}

// The finished list is in instance order, so learner p's episodes are the run [lo, hi) of it whose
// instances lie in [p b, (p + 1) b): two binary searches. With P = 1 and mz_ppo_scan's list (ids in
// [0, B), ascending) that is the whole list. The stores rely on that order also for one learner:
// an id out of range or out of order in the list can hide entries after it from the searches, and
// the ring then advances by hi - lo, not by the list's length.
__device__ __forceinline__ int drqn_first_at_least(const int32_t* a, const int n, const int64_t v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void drqn_pop_run(const int32_t* fin_id, const int32_t* fin_count,
                                             const int B, const int b, const int p, int* lo,
                                             int* hi) {
  const int nfin = min(max(*fin_count, 0), B);
  *lo = drqn_first_at_least(fin_id, nfin, (int64_t)p * b);
  *hi = drqn_first_at_least(fin_id, nfin, (int64_t)(p + 1) * b);
}
__device__ __forceinline__ void drqn_pop_run(const MzDrqnPopStore& q, const int p, int* lo,
                                             int* hi) {
  drqn_pop_run(q.s.fin_id, q.s.fin_count, q.s.B, q.b, p, lo, hi);
}

// workgroups (., p): learner p's run into learner p's ring. A learner with no finished episode
// writes nothing.
__global__ __launch_bounds__(256) void k_drqn_store(MzDrqnPopStore q) {
  const int p = blockIdx.y;
  int lo, hi;
  drqn_pop_run(q, p, &lo, &hi);
  if (hi <= lo) return;
  MzDrqnStore s = q.s;
  s.mem += (size_t)p * s.cap * (s.L + 1) * ROW;
  s.mem_len += (size_t)p * s.cap;
  s.mem_term += (size_t)p * s.cap;
  s.ring += 2 * (size_t)p;
  drqn_store_body(s, q.s.fin_id + lo, q.s.fin_len + lo, hi - lo, blockIdx.x, gridDim.x);
}

// after k_drqn_store (same stream): learner p's head and count move on by its stored episodes
__global__ __launch_bounds__(WAVE) void k_drqn_ring(MzDrqnPopStore q) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= q.P) return;
  int lo, hi;
  drqn_pop_run(q, p, &lo, &hi);
  if (hi > lo) drqn_ring_advance(q.s.ring + 2 * (size_t)p, hi - lo, q.s.cap);
}

// E distinct slots, every E-subset of the filled slots equally likely (Floyd): for j = n - E .. n - 1
// draw v uniform in [0, j]; take v unless already taken, else j. The draw is the high word of
// u32 * (j + 1) (bias below 2^-32 (j + 1)). While count < capacity the filled slots are 0 ..
// count - 1; afterwards all of them.
__device__ __forceinline__ void drqn_sample_body(const MzDrqnSample& q, int32_t* chosen) {
  const int lane = threadIdx.x;
  int64_t n64 = q.ring[1];
  if (n64 > q.cap) n64 = q.cap;
  const int n = (int)n64;
  if (n < q.E) {  // the host checked its own count: nothing to train on
    for (int e = lane; e < q.E; e += WAVE) {
      q.d_slot[e] = 0;
      q.d_len[e] = 0;
      q.d_off[e] = 0;
    }
    if (lane == 0) q.d_tot[0] = q.d_tot[1] = 0;
    return;
  }
  for (int m = 0; m < q.E; ++m) {
    const int j = n - q.E + m;
    uint32_t r[4];
    mz_philox(q.seed, MZ_DRQN_SAMPLE_STREAM ^ ((uint64_t)(uint32_t)m << 32), q.counter, r);
    const int v = (int)(((uint64_t)r[0] * (uint64_t)(j + 1)) >> 32);
    bool hit = false;
    for (int e = lane; e < m; e += WAVE) hit |= chosen[e] == v;
    const int pick = __any(hit) ? j : v;
    __syncthreads();
    if (lane == 0) chosen[m] = pick;
    __syncthreads();
  }
  if (lane == 0) {
    int64_t rows = 0, steps = 0;
    for (int e = 0; e < q.E; ++e) {
      const int s = chosen[e];
      int len = q.mem_len[s];
      if (len < 1 || len > q.L) len = 0;  // (never: the store writes 1..L)
      q.d_slot[e] = s;
      q.d_len[e] = len;
      q.d_off[e] = rows;
      rows += len + 1;
      steps += len;
    }
    q.d_tot[0] = rows;
    q.d_tot[1] = steps;
  }
}

// one wave per learner: the body on learner p's ring with its seed and update count
__global__ __launch_bounds__(WAVE) void k_drqn_sample(MzDrqnPopSample q) {
  extern __shared__ int32_t chosen[];  // [E]
  const int p = blockIdx.x;
  if (q.due && q.due[p] == 0) return;
  MzDrqnSample s = q.s;
  if (q.seed) s.seed = q.seed[p];
  if (q.counter) s.counter = q.counter[p];
  s.ring += 2 * (size_t)p;
  s.mem_len += (size_t)p * s.cap;
  s.d_slot += (size_t)p * s.E;
  s.d_len += (size_t)p * s.E;
  s.d_off += (size_t)p * s.E;
  s.d_tot += 2 * (size_t)p;
  drqn_sample_body(s, chosen);
}

// ---- the sequence forward --------------------------------------------------------------------
// A lane's share of the net in the sequence and window forwards: lane = (unit u, half) owns gate
// rows r0 = half 64 + u and r1 = r0 + 32, i.e. (i_u, f_u) or (g_u, o_u), and row lane & 3 of the head.
struct DrqnFwdLane {
  float b0, b1, wx0[NX], wx1[NX], wh0[H], wh1[H], fw[H], fb;
};
__device__ __forceinline__ void drqn_fwd_lane(const MzDrqnNet& p, const int lane, DrqnFwdLane& w) {
  const int r0 = (lane >> 5) * 2 * H + (lane & (H - 1)), r1 = r0 + H;
  w.b0 = p.b_ih[r0] + p.b_hh[r0];
  w.b1 = p.b_ih[r1] + p.b_hh[r1];
#pragma unroll
  for (int k = 0; k < NX; ++k) {
    w.wx0[k] = p.w_ih[r0 * NX + k];
    w.wx1[k] = p.w_ih[r1 * NX + k];
  }
#pragma unroll
  for (int k = 0; k < H; ++k) {
    w.wh0[k] = p.w_hh[r0 * H + k];
    w.wh1[k] = p.w_hh[r1 * H + k];
    w.fw[k] = p.fc_w[(lane & 3) * H + k];
  }
  w.fb = p.fc_b[lane & 3];
}

// One step of the cell from (hb = the old h, c) on the replay row (ra, rb): the lane's two gates
// after their nonlinearity (v0, v1), the new c and h of unit u, and the new h of every unit in hb
// (through hs, 128 B of LDS).
__device__ __forceinline__ void drqn_fwd_step(const DrqnFwdLane& w, const uint4 ra, const uint4 rb,
                                              float* hs, const int u, const int half,
                                              float (&hb)[H], float& c, float& h, float& v0,
                                              float& v1) {
  const float x[NX] = {__uint_as_float(ra.x), __uint_as_float(ra.y), __uint_as_float(ra.z),
                       __uint_as_float(ra.w), __uint_as_float(rb.x), __uint_as_float(rb.y)};
  float z0 = w.b0, z1 = w.b1;
#pragma unroll
  for (int k = 0; k < NX; ++k) {
    z0 = fmaf(w.wx0[k], x[k], z0);
    z1 = fmaf(w.wx1[k], x[k], z1);
  }
#pragma unroll
  for (int k = 0; k < H; ++k) {
    z0 = fmaf(w.wh0[k], hb[k], z0);
    z1 = fmaf(w.wh1[k], hb[k], z1);
  }
  v0 = half ? tanhf(z0) : sigmoidf_(z0);  // g or i
  v1 = sigmoidf_(z1);                     // o or f
  const float p0 = __shfl_xor(v0, 32), p1 = __shfl_xor(v1, 32);
  const float gi = half ? p0 : v0, gf = half ? p1 : v1, gg = half ? v0 : p0, go = half ? v1 : p1;
  c = gf * c + gi * gg;
  h = go * tanhf(c);
  __syncthreads();
  if (!half) hs[u] = h;
  __syncthreads();
#pragma unroll
  for (int k4 = 0; k4 < H / 4; ++k4) {
    const float4 v = reinterpret_cast<const float4*>(hs)[k4];
    hb[4 * k4 + 0] = v.x;
    hb[4 * k4 + 1] = v.y;
    hb[4 * k4 + 2] = v.z;
    hb[4 * k4 + 3] = v.w;
  }
}

// the four q values of the state in hb, in every lane
__device__ __forceinline__ void drqn_fwd_head(const DrqnFwdLane& w, const float (&hb)[H], float& q0,
                                              float& q1, float& q2, float& q3) {
  float qa = w.fb;  // q[lane & 3]
#pragma unroll
  for (int k = 0; k < H; ++k) qa = fmaf(w.fw[k], hb[k], qa);
  q0 = __shfl(qa, 0);
  q1 = __shfl(qa, 1);
  q2 = __shfl(qa, 2);
  q3 = __shfl(qa, 3);
}

// What one wave unrolls: steps b .. b + kb + m - 1 of the n-step episode in ring slot `slot`. The kb
// burn-in steps only advance the state; training step i is row `row + i` of the row buffers. A
// whole episode is b = kb = 0, m = n from zero state (snap null) with no entry row; a window
// starts from snapshot b / T (or zero) and keeps the state that enters its first training step in
// the row above `row` (entry).
struct DrqnSpan {
  int slot, n, b, kb, m;
  int64_t row;
  bool entry;
  const float* snap;
};

// The forward time loop of both update kinds. Target mode: max_a Q'_t of the m training steps and
// of the step after them (rows row .. row + m). Source mode: the stash, Q_t[a_t], y_t, the
// residual scaled by 2 / tot[1] and the span's sum of squared residuals (float64, time order).
// FORM is fixed at compile time. FWD_MAX is the two modes above, chosen by q.target. The other two
// serve double-Q targets and n-step returns, where y is formed afterwards (drqn_returns_body):
// FWD_Q4 is the target mode writing all four Q'_t of a row to x.q4 instead of their max; FWD_SEL
// the source mode that unrolls one step further (x_{s+m}, from its own state), writes the first
// argmax of its own Q_t to x.sel for rows row .. row + m, the stash and Q_t[a_t] for the training
// rows, and neither y, d nor ep_loss. The extra step has no stash row and no loss term.
enum { FWD_MAX = 0, FWD_Q4 = 1, FWD_SEL = 2 };
// whether the form runs the target mode's loop (FWD_MAX: the runtime flag, as before the forms)
template <int FORM>
__device__ __forceinline__ int drqn_fwd_target(const MzDrqnUnroll& q) {
  return FORM == FWD_Q4 ? 1 : (FORM == FWD_MAX ? q.target : 0);
}
template <int FORM>
__device__ __forceinline__ void drqn_unroll_fwd(const MzDrqnUnroll& q, const int e,
                                                const DrqnSpan& w, const int64_t* tot,
                                                const MzDrqnQRows& x) {
  __shared__ __attribute__((aligned(16))) float hs[H];
  const int lane = threadIdx.x, u = lane & (H - 1), half = lane >> 5;
  const uint32_t* ep = q.mem + ((size_t)w.slot * (q.L + 1) + w.b) * ROW;
  const int r0 = half * 2 * H + u, r1 = r0 + H;  // (i_u, f_u) or (g_u, o_u)
  DrqnFwdLane lw;
  drqn_fwd_lane(q.p, lane, lw);
  float hb[H];
#pragma unroll
  for (int k = 0; k < H; ++k) hb[k] = w.snap ? w.snap[k] : 0.0f;
  float c = w.snap ? w.snap[H + u] : 0.0f;
  float h = w.snap ? w.snap[u] : 0.0f;
  // (FWD_SEL runs the target mode's extra step and, as it, needs neither 1 / tot[1] nor term)
  const int steps = w.kb + w.m + (FORM == FWD_MAX ? (q.target ? 1 : 0) : 1);
  const float inv = FORM != FWD_MAX ? 0.0f : (q.target ? 0.0f : (float)(1.0 / (double)tot[1]));
  const bool term = FORM != FWD_MAX ? false : q.mem_term[w.slot] != 0;
  double sq = 0.0;
  for (int i = 0;; ++i) {
    // the state entering the first training step
    if (w.entry && !drqn_fwd_target<FORM>(q) && i == w.kb) {
      float* st = q.stash + (size_t)(w.row - 1) * STASH;
      if (!half) st[G4 + u] = c; else st[G4 + H + u] = h;
    }
    if (i >= steps) break;
    const uint4 ra = *reinterpret_cast<const uint4*>(ep + (size_t)i * ROW);
    const uint4 rb = *reinterpret_cast<const uint4*>(ep + (size_t)i * ROW + 4);
    float v0, v1, q0, q1, q2, q3;
    drqn_fwd_step(lw, ra, rb, hs, u, half, hb, c, h, v0, v1);
    if (i < w.kb) continue;  // burn-in: no q, no loss term
    drqn_fwd_head(lw, hb, q0, q1, q2, q3);
    const int64_t R = w.row + (i - w.kb);
    if (FORM == FWD_Q4) {
      if (lane == 0) reinterpret_cast<float4*>(x.q4)[R] = make_float4(q0, q1, q2, q3);
      continue;
    }
    if (FORM == FWD_SEL) {
      // the acting kernel's greedy rule: the first maximum; a NaN row selects 0
      const float qv[4] = {q0, q1, q2, q3};
      int a = 0;
#pragma unroll
      for (int k = 1; k < 4; ++k)
        if (qv[k] > qv[a]) a = k;
      if (lane == 0) x.sel[R] = a;
      if (i - w.kb >= w.m) continue;  // the step after the last training step
    }
    if (drqn_fwd_target<FORM>(q)) {
      if (lane == 0) q.qmax[R] = fmaxf(fmaxf(q0, q1), fmaxf(q2, q3));
      continue;
    }
    float* st = q.stash + (size_t)R * STASH;
    st[r0] = v0;
    st[r1] = v1;
    if (!half) st[G4 + u] = c; else st[G4 + H + u] = h;
    const int a = (int)rb.z & 3;
    const float rew = __uint_as_float(rb.w);
    const float qsel = a == 0 ? q0 : (a == 1 ? q1 : (a == 2 ? q2 : q3));
    if (FORM == FWD_SEL) {
      if (lane == 0) q.qa[R] = qsel;
      continue;
    }
    const bool last = w.b + i == w.n - 1;
    const float y = (last && term) ? rew : fmaf(q.gamma, q.qmax[R + 1], rew);
    const float d = qsel - y;
    sq += (double)d * (double)d;
    if (lane == 0) {
      q.qa[R] = qsel;
      q.y[R] = y;
      q.d[R] = 2.0f * d * inv;
    }
  }
  if (FORM == FWD_MAX && !drqn_fwd_target<FORM>(q) && lane == 0) q.ep_loss[e] = sq;
}

// learner p's view of what both update kinds share: its parameters, ring, discount factor and row
// buffers ([P][rows])
__device__ __forceinline__ void drqn_unroll_row(MzDrqnUnroll& s, const float* gamma, const int p,
                                                const size_t rows) {
  const size_t E = (size_t)s.E;
  s.p = drqn_net_row(s.p, p);
  if (gamma) s.gamma = gamma[p];
  s.mem += (size_t)p * s.cap * (s.L + 1) * ROW;
  if (s.mem_term) s.mem_term += (size_t)p * s.cap;
  if (s.qmax) s.qmax += p * rows;
  if (s.stash) s.stash += p * rows * STASH;
  if (s.qa) s.qa += p * rows;
  if (s.y) s.y += p * rows;
  if (s.d) s.d += p * rows;
  if (s.ep_loss) s.ep_loss += p * E;
  if (s.gpart) s.gpart += p * E * MZ_DRQN_PARAMS;
}

// learner p's view of a whole-episode update: also its directory ([P][E])
__device__ __forceinline__ MzDrqnSeq drqn_seq_row(const MzDrqnPopSeq& q, const int p) {
  MzDrqnSeq s = q.q;
  const size_t E = (size_t)s.u.E;
  drqn_unroll_row(s.u, q.gamma, p, E * (s.u.L + 1));
  s.d_slot += p * E;
  s.d_len += p * E;
  s.d_off += p * E;
  s.d_tot += 2 * (size_t)p;
  return s;
}

// episode e of the directory as a span; false where it is not one the sampler writes. Step t is
// row off + t, the target's q of step n row off + n.
__device__ __forceinline__ bool drqn_episode(const MzDrqnSeq& q, const int e, DrqnSpan* w) {
  const int n = q.d_len[e], slot = q.d_slot[e];
  const int64_t off = q.d_off[e];
  if (n < 1 || n > q.u.L || slot < 0 || slot >= q.u.cap || off < 0 ||
      off + n + 1 > (int64_t)q.u.E * (q.u.L + 1))
    return false;
  *w = DrqnSpan{slot, n, 0, 0, n, off, false, nullptr};
  return true;
}

// one wave per (learner, episode); a learner that is not due exits at once
__global__ __launch_bounds__(WAVE) void k_drqn_seq_fwd(MzDrqnPopSeq q) {
  const int p = blockIdx.x / q.q.u.E, e = blockIdx.x % q.q.u.E;
  if (q.due && q.due[p] == 0) return;
  const MzDrqnSeq s = drqn_seq_row(q, p);
  DrqnSpan w;
  if (drqn_episode(s, e, &w)) drqn_unroll_fwd<FWD_MAX>(s.u, e, w, s.d_tot, MzDrqnQRows{});
}

// ---- back-propagation through time -----------------------------------------------------------
// A lane's state in the sequence and window backwards (the forward's lane layout): the weights it
// reads, the gradient accumulators of its two gate rows and of the head, and what flows back in time.
struct DrqnBwdLane {
  float wt[2 * H], fcu[4];  // W_hh^T: unit u's column over the half's 64 gate rows; fc_w[:, u]
  float gx0[NX], gx1[NX], gh0[H], gh1[H], gfc[4], gfb[4], gb0, gb1;
  float dh_next, dc_next;
};
__device__ __forceinline__ void drqn_bwd_lane(const MzDrqnNet& p, const int u, const int half,
                                              DrqnBwdLane& g) {
#pragma unroll
  for (int j = 0; j < 2 * H; ++j) g.wt[j] = p.w_hh[(half * 2 * H + j) * H + u];
#pragma unroll
  for (int a = 0; a < 4; ++a) g.fcu[a] = p.fc_w[a * H + u];
#pragma unroll
  for (int k = 0; k < NX; ++k) g.gx0[k] = g.gx1[k] = 0.0f;
#pragma unroll
  for (int k = 0; k < H; ++k) g.gh0[k] = g.gh1[k] = 0.0f;
#pragma unroll
  for (int a = 0; a < 4; ++a) g.gfc[a] = g.gfb[a] = 0.0f;
  g.gb0 = g.gb1 = g.dh_next = g.dc_next = 0.0f;
}

// the (c, h) of the step one stash row above st: c of unit u, h of every unit
__device__ __forceinline__ void drqn_bwd_prev(const float* st, const int u, float& cp,
                                              float (&hp)[H]) {
  cp = st[G4 + u - STASH];
  const float4* hv = reinterpret_cast<const float4*>(st - STASH + G4 + H);
#pragma unroll
  for (int k4 = 0; k4 < H / 4; ++k4) {
    const float4 v = hv[k4];
    hp[4 * k4 + 0] = v.x;
    hp[4 * k4 + 1] = v.y;
    hp[4 * k4 + 2] = v.z;
    hp[4 * k4 + 3] = v.w;
  }
}

// One step back: from the step's stash row st, the state before it (cp, hp), its replay row and
// d = d loss / d Q_t[a_t] (the 1 / steps folded in) the lane's gradient terms, dc_{t-1} and dh_{t-1}
// (through dzs, 512 B of LDS).
__device__ __forceinline__ void drqn_bwd_step(DrqnBwdLane& g, const float* st, const float cp,
                                              const float (&hp)[H], const uint4 ra, const uint4 rb,
                                              const float d, float* dzs, const int u,
                                              const int half) {
  const int r0 = half * 2 * H + u, r1 = r0 + H;
  const float gi = st[u], gf = st[H + u], gg = st[2 * H + u], go = st[3 * H + u];
  const float ct = st[G4 + u], ht = st[G4 + H + u];
  const float x[NX] = {__uint_as_float(ra.x), __uint_as_float(ra.y), __uint_as_float(ra.z),
                       __uint_as_float(ra.w), __uint_as_float(rb.x), __uint_as_float(rb.y)};
  const int a = (int)rb.z & 3;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    g.gfc[k] += k == a ? d * ht : 0.0f;
    g.gfb[k] += k == a ? d : 0.0f;
  }
  const float fsel = a == 0 ? g.fcu[0] : (a == 1 ? g.fcu[1] : (a == 2 ? g.fcu[2] : g.fcu[3]));
  const float dh = fmaf(d, fsel, g.dh_next);
  const float tc = tanhf(ct);
  const float dc = fmaf(dh * go, 1.0f - tc * tc, g.dc_next);
  const float dzi = dc * gg * gi * (1.0f - gi);
  const float dzf = dc * cp * gf * (1.0f - gf);
  const float dzg = dc * gi * (1.0f - gg * gg);
  const float dzo = dh * tc * go * (1.0f - go);
  g.dc_next = dc * gf;
  const float dz0 = half ? dzg : dzi, dz1 = half ? dzo : dzf;
  g.gb0 += dz0;
  g.gb1 += dz1;
#pragma unroll
  for (int k = 0; k < NX; ++k) {
    g.gx0[k] = fmaf(dz0, x[k], g.gx0[k]);
    g.gx1[k] = fmaf(dz1, x[k], g.gx1[k]);
  }
#pragma unroll
  for (int k = 0; k < H; ++k) {
    g.gh0[k] = fmaf(dz0, hp[k], g.gh0[k]);
    g.gh1[k] = fmaf(dz1, hp[k], g.gh1[k]);
  }
  // dh_{t-1}[u] = sum over the 128 gate rows of W_hh[row][u] dz[row]: each half its 64 rows in
  // row order, then the two halves added
  __syncthreads();
  dzs[r0] = dz0;
  dzs[r1] = dz1;
  __syncthreads();
  float part = 0.0f;
#pragma unroll
  for (int j4 = 0; j4 < 2 * H / 4; ++j4) {
    const float4 v = reinterpret_cast<const float4*>(dzs + half * 2 * H)[j4];
    part = fmaf(g.wt[4 * j4 + 0], v.x, part);
    part = fmaf(g.wt[4 * j4 + 1], v.y, part);
    part = fmaf(g.wt[4 * j4 + 2], v.z, part);
    part = fmaf(g.wt[4 * j4 + 3], v.w, part);
  }
  g.dh_next = part + __shfl_xor(part, 32);
}

// the lane's accumulators into the partial gp [5252], flat parameter order
__device__ __forceinline__ void drqn_bwd_write(const DrqnBwdLane& g, float* gp, const int lane) {
  const int u = lane & (H - 1), half = lane >> 5;
  const int r0 = half * 2 * H + u, r1 = r0 + H;
#pragma unroll
  for (int k = 0; k < NX; ++k) {
    gp[P_WIH + r0 * NX + k] = g.gx0[k];
    gp[P_WIH + r1 * NX + k] = g.gx1[k];
  }
#pragma unroll
  for (int k = 0; k < H; ++k) {
    gp[P_WHH + r0 * H + k] = g.gh0[k];
    gp[P_WHH + r1 * H + k] = g.gh1[k];
  }
  gp[P_BIH + r0] = g.gb0;
  gp[P_BIH + r1] = g.gb1;
  gp[P_BHH + r0] = g.gb0;
  gp[P_BHH + r1] = g.gb1;
  if (!half) {
#pragma unroll
    for (int a = 0; a < 4; ++a) gp[P_FCW + a * H + u] = g.gfc[a];
  }
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 4; ++a) gp[P_FCB + a] = g.gfb[a];
  }
}

// the partial of a span that is not one the sampler writes
__device__ __forceinline__ void drqn_zero_partial(float* gp) {
  for (int k = threadIdx.x; k < MZ_DRQN_PARAMS; k += WAVE) gp[k] = 0.0f;
}

// The backward time loop of both update kinds: BPTT over the span's m training steps into partial
// e. Every step finds (c, h) of its predecessor one row up; the first step's is the entry row, or
// zero where there is none. Nothing flows into the burn-in.
__device__ __forceinline__ void drqn_unroll_bwd(const MzDrqnUnroll& q, const int e,
                                                const DrqnSpan& w) {
  __shared__ __attribute__((aligned(16))) float dzs[G4];
  const int lane = threadIdx.x, u = lane & (H - 1), half = lane >> 5;
  const uint32_t* ep = q.mem + ((size_t)w.slot * (q.L + 1) + w.b + w.kb) * ROW;
  DrqnBwdLane g;
  drqn_bwd_lane(q.p, u, half, g);
  for (int t = w.m - 1; t >= 0; --t) {
    const int64_t R = w.row + t;
    const float* st = q.stash + (size_t)R * STASH;
    float cp = 0.0f, hp[H];
    if (t || w.entry) {
      drqn_bwd_prev(st, u, cp, hp);
    } else {
#pragma unroll
      for (int k = 0; k < H; ++k) hp[k] = 0.0f;
    }
    const uint4 ra = *reinterpret_cast<const uint4*>(ep + (size_t)t * ROW);
    const uint4 rb = *reinterpret_cast<const uint4*>(ep + (size_t)t * ROW + 4);
    drqn_bwd_step(g, st, cp, hp, ra, rb, q.d[R], dzs, u, half);
  }
  drqn_bwd_write(g, q.gpart + (size_t)e * MZ_DRQN_PARAMS, lane);
}

__global__ __launch_bounds__(WAVE) void k_drqn_seq_bwd(MzDrqnPopSeq q) {
  const int p = blockIdx.x / q.q.u.E, e = blockIdx.x % q.q.u.E;
  if (q.due && q.due[p] == 0) return;
  const MzDrqnSeq s = drqn_seq_row(q, p);
  DrqnSpan w;
  if (!drqn_episode(s, e, &w)) {
    drqn_zero_partial(s.u.gpart + (size_t)e * MZ_DRQN_PARAMS);
    return;
  }
  drqn_unroll_bwd(s.u, e, w);
}

// parameter k's partials summed over the episodes in index order (float64, rounded once)
__device__ __forceinline__ float drqn_reduce_grad(const float* gpart, const int E, const int k) {
  double s = 0.0;
  for (int e = 0; e < E; ++e) s += (double)gpart[(size_t)e * MZ_DRQN_PARAMS + k];
  return (float)s;
}

// the loss: the episodes' sums of squared residuals in episode order (float64) over the steps
__device__ __forceinline__ float drqn_reduce_loss(const double* ep_loss, const int32_t* d_len,
                                                  const int64_t* d_tot, const int E) {
  double s = 0.0;
  for (int e = 0; e < E; ++e)
    if (d_len[e] > 0) s += ep_loss[e];
  const int64_t steps = d_tot[1];
  return steps > 0 ? (float)(s / (double)steps) : 0.0f;
}

// workgroups (., p): learner p's E partials into its six gradient segments (learner 0's, moved by
// p rows of the flat [P][5252] gradient), and its loss. Learner p's lengths are d_len + p ld:
// ld = E for the [P][E] episode directory, 5 E for the m row of the [P][5][E] window directory.
__global__ __launch_bounds__(256) void k_drqn_reduce(MzDrqnReduce q) {
  const int p = blockIdx.y;
  if (q.due && q.due[p] == 0) return;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t E = (size_t)q.E;
  if (k < MZ_DRQN_PARAMS) {
    const float s = drqn_reduce_grad(q.gpart + p * E * MZ_DRQN_PARAMS, q.E, k);
    float* dst;
    int o;
    if (k < P_WHH) { dst = q.g.w_ih; o = k - P_WIH; }
    else if (k < P_BIH) { dst = q.g.w_hh; o = k - P_WHH; }
    else if (k < P_BHH) { dst = q.g.b_ih; o = k - P_BIH; }
    else if (k < P_FCW) { dst = q.g.b_hh; o = k - P_BHH; }
    else if (k < P_FCB) { dst = q.g.fc_w; o = k - P_FCW; }
    else { dst = q.g.fc_b; o = k - P_FCB; }
    dst[(size_t)p * MZ_DRQN_PARAMS + o] = s;
  }
  if (k == 0)
    q.loss[p] = drqn_reduce_loss(q.ep_loss + p * E, q.d_len + (size_t)p * q.ld,
                                 q.d_tot + 2 * (size_t)p, q.E);
}

// the target sync of the learners flagged in mask: dst row <- src row
__global__ __launch_bounds__(256) void k_drqn_pop_sync(const float* __restrict__ src,
                                                       float* __restrict__ dst,
                                                       const int32_t* __restrict__ mask) {
  const int p = blockIdx.y;
  if (mask[p] == 0) return;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < MZ_DRQN_PARAMS) dst[(size_t)p * MZ_DRQN_PARAMS + k] = src[(size_t)p * MZ_DRQN_PARAMS + k];
}

// ---- replay windows: stored state, burn-in -------------------------------------------------
constexpr int SNAP = MZ_DRQN_SNAP;  // h[32], c[32]
__device__ __forceinline__ int drqn_windows(const int n, const int T) { return (n - 1) / T + 1; }

// Before the acting step: where 0 < t[i] < L and t[i] % T == 0 the state instance i is about to
// act from goes to its in-flight record as snapshot t[i] / T. Workgroups (., w): word w of 256
// instances, so the reads of h / c ([32][B]) coalesce; one instance in T writes.
__global__ __launch_bounds__(256) void k_drqn_snapshot(MzDrqnSnap q) {
  const int i = blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
  if (i >= q.B) return;
  const int t = q.t[i];
  if (t <= 0 || t >= q.L || t % q.T != 0) return;
  const float v = w < H ? q.h[(size_t)w * q.B + i] : q.c[(size_t)(w - H) * q.B + i];
  q.snap_rec[((size_t)i * drqn_windows(q.L, q.T) + t / q.T) * SNAP + w] = v;
}

// Before k_drqn_store (which advances the ring): the listed episodes' snapshots 1 ..
// ceil(n / T) - 1 into the slot k_drqn_store gives the episode, by the same rule.
// The listed episodes fin_id / fin_len [0, nfin) as drqn_store_body takes them; workgroup blk of
// nblk takes every nblk-th.
__device__ __forceinline__ void drqn_snap_store_body(const MzDrqnSnapStore& q,
                                                     const int32_t* fin_id, const int32_t* fin_len,
                                                     const int nfin, const int blk,
                                                     const int nblk) {
  const int64_t head = q.ring[0];
  const size_t per = (size_t)drqn_windows(q.L, q.T) * SNAP;
  const int first = nfin > q.cap ? nfin - (int)q.cap : 0;
  for (int k = first + blk; k < nfin; k += nblk) {
    const int i = fin_id[k], n = fin_len[k];
    if (i < 0 || i >= q.B || n < 1 || n > q.L || head < 0 || head >= q.cap) continue;
    const int64_t slot = (head + k) % q.cap;
    const float* src = q.snap_rec + (size_t)i * per;
    float* dst = q.mem_state + (size_t)slot * per;
    for (int e = SNAP + threadIdx.x; e < drqn_windows(n, q.T) * SNAP; e += blockDim.x)
      dst[e] = src[e];
  }
}

// workgroups (., p), before k_drqn_store: learner p's run of the finished list (k_drqn_store's
// run) with its ring and its state memory; snap_rec stays indexed by the global instance. A
// learner with no finished episode writes nothing.
__global__ __launch_bounds__(256) void k_drqn_snap_store(MzDrqnPopSnapStore q) {
  const int p = blockIdx.y;
  int lo, hi;
  drqn_pop_run(q.s.fin_id, q.s.fin_count, q.s.B, q.b, p, &lo, &hi);
  if (hi <= lo) return;
  MzDrqnSnapStore s = q.s;
  s.mem_state += (size_t)p * s.cap * drqn_windows(s.L, s.T) * SNAP;
  s.ring += 2 * (size_t)p;
  drqn_snap_store_body(s, q.s.fin_id + lo, q.s.fin_len + lo, hi - lo, blockIdx.x, gridDim.x);
}

// k_drqn_sample's slots (the same draws), then per chosen episode one window j uniform over its
// ceil(n / T) windows (a Philox stream of its own, keyed by the position in the batch), the window
// directory and the row offsets: window e owns rows w_off[e] .. w_off[e] + m + 1. K < 0 (never
// from the host, which refuses it: a population learner whose device-side burn-in breaks the rule)
// gives the batch no window: b = k = m = 0 throughout.
__device__ __forceinline__ void drqn_win_sample_body(const MzDrqnWinSample& q, int32_t* chosen) {
  drqn_sample_body(q.s, chosen);
  __syncthreads();
  const int lane = threadIdx.x, E = q.s.E;
  int32_t* w = q.wdir;
  for (int e = lane; e < E; e += WAVE) {
    const int n = w[MZ_DRQN_WDIR_LEN * E + e];
    int b = 0, kb = 0, m = 0;
    if (n >= 1 && q.K >= 0) {
      uint32_t r[4];
      mz_philox(q.s.seed, MZ_DRQN_WINDOW_STREAM ^ ((uint64_t)(uint32_t)e << 32), q.s.counter, r);
      const int j = (int)(((uint64_t)r[0] * (uint64_t)drqn_windows(n, q.T)) >> 32);
      const int s = j * q.T;
      b = s > q.K ? s - q.K : 0;
      kb = s - b;
      m = min(q.T, n - s);
    }
    w[MZ_DRQN_WDIR_B * E + e] = b;
    w[MZ_DRQN_WDIR_K * E + e] = kb;
    w[MZ_DRQN_WDIR_M * E + e] = m;
  }
  __syncthreads();
  if (lane == 0) {
    int64_t rows = 0, steps = 0;
    for (int e = 0; e < E; ++e) {
      const int m = w[MZ_DRQN_WDIR_M * E + e];
      q.s.d_off[e] = rows;
      rows += m > 0 ? m + MZ_DRQN_WIN_PAD : 0;
      steps += m;
    }
    q.s.d_tot[0] = rows;
    q.s.d_tot[1] = steps;
  }
}

// learner p's burn-in where it keeps the rule (0 <= K_p <= K_max, a multiple of T), else -1, which
// no window passes: the sampler then writes none and drqn_window refuses every one
__device__ __forceinline__ int drqn_pop_burn_in(const int32_t* burn_in, const int p, const int T,
                                                const int Kmax) {
  const int K = burn_in[p];
  return (K >= 0 && K <= Kmax && K % T == 0) ? K : -1;
}

// one wave per learner: the body on learner p's ring with its seed, update count and burn-in, and
// its directory block [5][E]
__global__ __launch_bounds__(WAVE) void k_drqn_win_sample(MzDrqnPopWinSample q) {
  extern __shared__ int32_t chosen[];  // [E]
  const int p = blockIdx.x;
  if (q.due && q.due[p] == 0) return;
  MzDrqnWinSample w = q.w;
  const size_t E = (size_t)w.s.E;
  if (q.burn_in) w.K = drqn_pop_burn_in(q.burn_in, p, w.T, q.w.K);
  w.wdir += (size_t)p * 5 * E;
  if (q.seed) w.s.seed = q.seed[p];
  if (q.counter) w.s.counter = q.counter[p];
  w.s.ring += 2 * (size_t)p;
  w.s.mem_len += (size_t)p * w.s.cap;
  w.s.d_slot = w.wdir + MZ_DRQN_WDIR_SLOT * E;
  w.s.d_len = w.wdir + MZ_DRQN_WDIR_LEN * E;
  w.s.d_off += p * E;
  w.s.d_tot += 2 * (size_t)p;
  drqn_win_sample_body(w, chosen);
}

// Window e of the directory as a span; false where it is not one the sampler writes. Rows: the
// window's first row (w_off) holds (c, h) entering the first training step, where the backward
// finds them; training step i is row w_off + 1 + i; the target's q of step b + kb + m is in the
// guard row. The entry state is snapshot b / T, zero where b == 0 or there is no state memory.
__device__ __forceinline__ bool drqn_window(const MzDrqnWin& q, const int e, DrqnSpan* w) {
  const int E = q.u.E;
  w->slot = q.wdir[MZ_DRQN_WDIR_SLOT * E + e];
  w->n = q.wdir[MZ_DRQN_WDIR_LEN * E + e];
  w->b = q.wdir[MZ_DRQN_WDIR_B * E + e];
  w->kb = q.wdir[MZ_DRQN_WDIR_K * E + e];
  w->m = q.wdir[MZ_DRQN_WDIR_M * E + e];
  const int64_t off = q.w_off[e];
  w->row = off + 1;
  w->entry = true;
  const int64_t rows = (int64_t)E * (min(q.T, q.u.L) + MZ_DRQN_WIN_PAD);
  if (!(w->n >= 1 && w->n <= q.u.L && w->slot >= 0 && w->slot < q.u.cap && w->m >= 1 &&
        w->m <= q.T && w->b >= 0 && w->b % q.T == 0 && w->kb >= 0 && w->kb <= q.K &&
        (int64_t)w->b + w->kb + w->m <= w->n && off >= 0 && off + w->m + MZ_DRQN_WIN_PAD <= rows))
    return false;
  w->snap = (q.mem_state && w->b > 0)
      ? q.mem_state + ((size_t)w->slot * drqn_windows(q.u.L, q.T) + w->b / q.T) * SNAP : nullptr;
  return true;
}

// learner p's view of a population's windowed update: also its state memory (only where
// stored[p] != 0: otherwise zero state), directory block ([P][5][E]) and burn-in
__device__ __forceinline__ MzDrqnWin drqn_win_row(const MzDrqnPopWin& q, const int p) {
  MzDrqnWin s = q.q;
  const size_t E = (size_t)s.u.E;
  drqn_unroll_row(s.u, q.gamma, p, E * (min(s.T, s.u.L) + MZ_DRQN_WIN_PAD));
  if (q.burn_in) s.K = drqn_pop_burn_in(q.burn_in, p, s.T, q.q.K);
  if (s.mem_state)
    s.mem_state = (q.stored && q.stored[p] == 0)
        ? nullptr : s.mem_state + (size_t)p * s.u.cap * drqn_windows(s.u.L, s.T) * SNAP;
  s.wdir += p * 5 * E;
  s.w_off += p * E;
  s.w_tot += 2 * (size_t)p;
  return s;
}

// one wave per (learner, window); a learner that is not due exits at once
__global__ __launch_bounds__(WAVE) void k_drqn_win_fwd(MzDrqnPopWin q) {
  const int p = blockIdx.x / q.q.u.E, e = blockIdx.x % q.q.u.E;
  if (q.due && q.due[p] == 0) return;
  const MzDrqnWin s = drqn_win_row(q, p);
  DrqnSpan w;
  if (drqn_window(s, e, &w)) drqn_unroll_fwd<FWD_MAX>(s.u, e, w, s.w_tot, MzDrqnQRows{});
}

__global__ __launch_bounds__(WAVE) void k_drqn_win_bwd(MzDrqnPopWin q) {
  const int p = blockIdx.x / q.q.u.E, e = blockIdx.x % q.q.u.E;
  if (q.due && q.due[p] == 0) return;
  const MzDrqnWin s = drqn_win_row(q, p);
  DrqnSpan w;
  if (!drqn_window(s, e, &w)) {
    drqn_zero_partial(s.u.gpart + (size_t)e * MZ_DRQN_PARAMS);
    return;
  }
  drqn_unroll_bwd(s.u, e, w);
}

// ---- double-Q targets and n-step returns ---------------------------------------------------
// The update's chain when a learner leaves the defaults: the target forward in FWD_Q4, the source
// forward in FWD_SEL, then k_drqn_*_ret, which forms y, d and ep_loss; the priority update and the
// backward follow unchanged. The old forwards are not part of that chain and keep their code.
template <int FORM>
__global__ __launch_bounds__(WAVE) void k_drqn_seq_fwd_q(MzDrqnPopSeqQ q) {
  const int E = q.q.q.u.E, p = blockIdx.x / E, e = blockIdx.x % E;
  if (q.q.due && q.q.due[p] == 0) return;
  const MzDrqnSeq s = drqn_seq_row(q.q, p);
  const size_t rows = (size_t)E * (s.u.L + 1);
  const MzDrqnQRows x{q.x.q4 ? q.x.q4 + p * rows * 4 : nullptr, q.x.sel ? q.x.sel + p * rows : nullptr};
  DrqnSpan w;
  if (drqn_episode(s, e, &w)) drqn_unroll_fwd<FORM>(s.u, e, w, s.d_tot, x);
}

template <int FORM>
__global__ __launch_bounds__(WAVE) void k_drqn_win_fwd_q(MzDrqnPopWinQ q) {
  const int E = q.q.q.u.E, p = blockIdx.x / E, e = blockIdx.x % E;
  if (q.q.due && q.q.due[p] == 0) return;
  const MzDrqnWin s = drqn_win_row(q.q, p);
  const size_t rows = (size_t)E * (min(s.T, s.u.L) + MZ_DRQN_WIN_PAD);
  const MzDrqnQRows x{q.x.q4 ? q.x.q4 + p * rows * 4 : nullptr, q.x.sel ? q.x.sel + p * rows : nullptr};
  DrqnSpan w;
  if (drqn_window(s, e, &w)) drqn_unroll_fwd<FORM>(s.u, e, w, s.w_tot, x);
}

// One wave per span, after both forwards. Lane i takes training rows i, i + 64, ...: for training
// step t = s + i (s = b + kb) the return runs over k = min(N, m - i) rewards, up to step u = t + k,
// which the span's end cuts: no reward past row m - 1 is read, and the rows of q4 and sel end with
// the guard row. In float32 and in this order:
//   acc = no_boot ? r_{u-1} : fmaf(gamma, boot, r_{u-1});  acc = fmaf(gamma, acc, r_j), j = u-2 .. t
// boot = q4[u][sel[u]] when the learner is double, else max_a q4[u][a] (the old forward's fmaxf
// tree); no_boot where u is the end of a terminated episode. y = acc, d = 2 (qa - y) / tot[1], and
// ep_loss[e] the float64 sum of the squared residuals in time order, each round of 64 rows taken
// lane by lane (drqn_prio_update_body's idiom). N = 1 is the old source forward's arithmetic, op
// for op. No atomics.
__device__ __forceinline__ void drqn_returns_body(const MzDrqnUnroll& q, const float* q4,
                                                  const int32_t* sel, const int N, const int e,
                                                  const DrqnSpan& w, const int64_t* tot) {
  const int lane = threadIdx.x;
  const int s = w.b + w.kb;
  const uint32_t* ep = q.mem + ((size_t)w.slot * (q.L + 1) + s) * ROW;  // row i: training step i
  const float inv = (float)(1.0 / (double)tot[1]);
  const bool term = q.mem_term[w.slot] != 0;
  double sq = 0.0;
  for (int i0 = 0; i0 < w.m; i0 += WAVE) {
    const int i = i0 + lane;
    float d = 0.0f;
    if (i < w.m) {
      const int u = i + min(N, w.m - i);  // 1 .. m, relative to s
      float acc = __uint_as_float(ep[(size_t)(u - 1) * ROW + 7]);
      if (!(s + u == w.n && term)) {
        const int64_t Ru = w.row + u;
        const float4 v = reinterpret_cast<const float4*>(q4)[Ru];
        float boot;
        if (sel) {
          const int a = sel[Ru] & 3;
          boot = a == 0 ? v.x : (a == 1 ? v.y : (a == 2 ? v.z : v.w));
        } else {
          boot = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
        }
        acc = fmaf(q.gamma, boot, acc);
      }
      for (int j = u - 2; j >= i; --j)
        acc = fmaf(q.gamma, acc, __uint_as_float(ep[(size_t)j * ROW + 7]));
      const int64_t R = w.row + i;
      d = q.qa[R] - acc;
      q.y[R] = acc;
      q.d[R] = 2.0f * d * inv;
    }
    const int cnt = min(WAVE, w.m - i0);
    for (int j = 0; j < cnt; ++j) {
      const float v = __shfl(d, j);
      sq += (double)v * (double)v;
    }
  }
  if (lane == 0) q.ep_loss[e] = sq;
}

// learner p's n, rows of q4 and (where it is double) of sel
__device__ __forceinline__ int drqn_returns_row(const MzDrqnReturns& r, const int p,
                                                const size_t rows, const float** q4,
                                                const int32_t** sel) {
  *q4 = r.q4 + p * rows * 4;
  *sel = (r.sel && (!r.dbl || r.dbl[p] != 0)) ? r.sel + p * rows : nullptr;
  return min(max(r.n_step[p], 1), r.n_max);
}

__global__ __launch_bounds__(WAVE) void k_drqn_seq_ret(MzDrqnPopSeqRet q) {
  const int E = q.q.q.u.E, p = blockIdx.x / E, e = blockIdx.x % E;
  if (q.q.due && q.q.due[p] == 0) return;
  const MzDrqnSeq s = drqn_seq_row(q.q, p);
  const float* q4;
  const int32_t* sel;
  const int N = drqn_returns_row(q.r, p, (size_t)E * (s.u.L + 1), &q4, &sel);
  DrqnSpan w;
  if (drqn_episode(s, e, &w)) drqn_returns_body(s.u, q4, sel, N, e, w, s.d_tot);
}

__global__ __launch_bounds__(WAVE) void k_drqn_win_ret(MzDrqnPopWinRet q) {
  const int E = q.q.q.u.E, p = blockIdx.x / E, e = blockIdx.x % E;
  if (q.q.due && q.q.due[p] == 0) return;
  const MzDrqnWin s = drqn_win_row(q.q, p);
  const float* q4;
  const int32_t* sel;
  const int N = drqn_returns_row(q.r, p, (size_t)E * (min(s.T, s.u.L) + MZ_DRQN_WIN_PAD), &q4, &sel);
  DrqnSpan w;
  if (drqn_window(s, e, &w)) drqn_returns_body(s.u, q4, sel, N, e, w, s.w_tot);
}

// ---- prioritized replay windows ------------------------------------------------------------
// Masses are u32 fixed point (MZ_DRQN_PRIO_FRAC fractional bits), every sum over them an exact
// u64: whatever order a scan or a reduction below takes, its result is the integer the host model
// computes. The entry points bound cap W E 2^30 below 2^63, so no sum or product here wraps.
constexpr int PRIO_T = 1024;             // threads of the sampler and of the write-back
constexpr int PRIO_WAVES = PRIO_T / WAVE;

// inclusive scan over the wave's 64 lanes
__device__ __forceinline__ uint64_t drqn_wave_scan(uint64_t v, const int lane) {
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const unsigned long long u = __shfl_up((unsigned long long)v, o);
    if (lane >= o) v += u;
  }
  return v;
}

// The lane-parallel search both levels of the sampler use: n masses at a[0 .. n) (u64 or u32),
// 64 per round, taken in index order on top of `base`. Returns the index i with prefix(i) <= t <
// prefix(i) + a[i] and leaves prefix(i) in base; -1 (base = the whole sum added) where t lies
// beyond them all. Every lane of the wave gets the same answer.
template <class M>
__device__ __forceinline__ int64_t drqn_prio_find(const M* a, const int64_t n, const uint64_t t,
                                                  uint64_t& base, const int lane) {
  for (int64_t i0 = 0; i0 < n; i0 += WAVE) {
    const uint64_t v = i0 + lane < n ? (uint64_t)a[i0 + lane] : 0;
    const uint64_t inc = drqn_wave_scan(v, lane);
    const unsigned long long hit = __ballot(t < base + inc);
    if (hit) {
      const int l = __ffsll(hit) - 1;
      base += (uint64_t)__shfl((unsigned long long)(inc - v), l);
      return i0 + l;
    }
    base += (uint64_t)__shfl((unsigned long long)inc, WAVE - 1);
  }
  return -1;
}

// Entry: before k_drqn_store, by its slot rule and its validity tests: the listed episode of n
// steps gives its ceil(n / T) windows the mass prio_max, zero to the slot's other entries, and the
// slot its sum.
__device__ __forceinline__ void drqn_prio_store_body(const MzDrqnPrioStore& q,
                                                     const int32_t* fin_id, const int32_t* fin_len,
                                                     const int nfin, const int blk,
                                                     const int nblk) {
  const int64_t head = q.ring[0];
  const int W = drqn_windows(q.L, q.T);
  const uint32_t pm = q.prio_max[0];
  const int first = nfin > q.cap ? nfin - (int)q.cap : 0;
  for (int k = first + blk; k < nfin; k += nblk) {
    const int i = fin_id[k], n = fin_len[k];
    if (i < 0 || i >= q.B || n < 1 || n > q.L || head < 0 || head >= q.cap) continue;
    const int64_t slot = (head + k) % q.cap;
    const int nw = drqn_windows(n, q.T);
    for (int j = threadIdx.x; j < W; j += blockDim.x)
      q.mem_prio[(size_t)slot * W + j] = j < nw ? pm : 0u;
    if (threadIdx.x == 0) q.mem_psum[slot] = (uint64_t)nw * pm;
  }
}

__global__ __launch_bounds__(WAVE) void k_drqn_prio_store(MzDrqnPopPrioStore q) {
  const int p = blockIdx.y;
  int lo, hi;
  drqn_pop_run(q.s.fin_id, q.s.fin_count, q.s.B, q.b, p, &lo, &hi);
  if (hi <= lo) return;
  MzDrqnPrioStore s = q.s;
  s.mem_prio += (size_t)p * s.cap * drqn_windows(s.L, s.T);
  s.mem_psum += (size_t)p * s.cap;
  s.prio_max += p;
  s.ring += 2 * (size_t)p;
  drqn_prio_store_body(s, q.s.fin_id + lo, q.s.fin_len + lo, hi - lo, blockIdx.x, gridDim.x);
}

// Sampling, with replacement and stratified: S = the sum of all masses; position e draws t in
// [floor(e S / E), floor((e + 1) S / E)) and takes the window (slot, j) whose span of the
// slot-major, j-minor prefix holds t. The slots are cut into at most PRIO_T groups of 64 g
// consecutive slots: (1) every wave sums whole groups with coalesced loads; (2) one block scan
// turns the group sums into prefixes in LDS; (3) a wave per position finds its group by binary
// search, the slot inside the group and the window inside the slot by drqn_prio_find; (4) the
// smallest sampled mass (an integer atomic min in LDS), the weights, and the row offsets as
// drqn_win_sample_body lays them out. K < 0 gives the batch no window, as there.
__device__ __forceinline__ void drqn_prio_sample_body(const MzDrqnPrioSample& q) {
  __shared__ uint64_t gpre[PRIO_T];    // group sums, then their exclusive prefixes
  __shared__ uint64_t wsum[PRIO_WAVES];
  __shared__ uint32_t mmin;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int E = q.E, W = drqn_windows(q.L, q.T);
  const int64_t gsz = (int64_t)WAVE * ((q.cap + (int64_t)WAVE * PRIO_T - 1) / ((int64_t)WAVE * PRIO_T));
  const int ng = (int)((q.cap + gsz - 1) / gsz);  // <= PRIO_T
  for (int g = wave; g < ng; g += PRIO_WAVES) {
    uint64_t s = 0;
    const int64_t end = min((int64_t)(g + 1) * gsz, q.cap);
    for (int64_t i = (int64_t)g * gsz + lane; i < end; i += WAVE) s += q.mem_psum[i];
    s = drqn_wave_scan(s, lane);
    if (lane == WAVE - 1) gpre[g] = s;
  }
  if (tid == 0) mmin = 0xffffffffu;
  __syncthreads();
  const uint64_t own = tid < ng ? gpre[tid] : 0;
  const uint64_t inc = drqn_wave_scan(own, lane);
  if (lane == WAVE - 1) wsum[wave] = inc;
  __syncthreads();
  uint64_t before = 0, S = 0;
  for (int w = 0; w < PRIO_WAVES; ++w) {
    if (w < wave) before += wsum[w];
    S += wsum[w];
  }
  gpre[tid] = before + inc - own;
  __syncthreads();
  int32_t* wd = q.wdir;
  for (int e = wave; e < E; e += PRIO_WAVES) {
    int slot = 0, n = 0, b = 0, kb = 0, m = 0;
    if (S > 0 && q.K >= 0) {
      const uint64_t lo = (uint64_t)e * S / (uint64_t)E, hi = (uint64_t)(e + 1) * S / (uint64_t)E;
      uint32_t r[4];
      mz_philox(q.seed, MZ_DRQN_PRIO_STREAM ^ ((uint64_t)(uint32_t)e << 32), q.counter, r);
      const uint64_t t = lo + __umul64hi(((uint64_t)r[0] << 32) | r[1], hi - lo);
      int g = 0;  // the last group whose prefix is <= t: the one whose span holds t
      for (int step = PRIO_T / 2; step >= 1; step >>= 1)
        if (g + step < ng && gpre[g + step] <= t) g += step;
      uint64_t base = gpre[g];
      const int64_t s0 = (int64_t)g * gsz;
      const int64_t si = drqn_prio_find(q.mem_psum + s0, min(gsz, q.cap - s0), t, base, lane);
      if (si >= 0) {
        const int64_t sl = s0 + si;
        const int64_t j = drqn_prio_find(q.mem_prio + (size_t)sl * W, W, t, base, lane);
        const int len = q.mem_len[sl];
        if (j >= 0 && len >= 1 && len <= q.L && j < drqn_windows(len, q.T)) {
          const int s = (int)j * q.T;
          slot = (int)sl;
          n = len;
          b = s > q.K ? s - q.K : 0;
          kb = s - b;
          m = min(q.T, n - s);
        }
      }
    }
    if (lane == 0) {
      wd[MZ_DRQN_WDIR_SLOT * E + e] = slot;
      wd[MZ_DRQN_WDIR_LEN * E + e] = n;
      wd[MZ_DRQN_WDIR_B * E + e] = b;
      wd[MZ_DRQN_WDIR_K * E + e] = kb;
      wd[MZ_DRQN_WDIR_M * E + e] = m;
      if (m > 0) atomicMin(&mmin, q.mem_prio[(size_t)slot * W + (b + kb) / q.T]);
    }
  }
  __syncthreads();
  for (int e = tid; e < E; e += PRIO_T) {
    float w = 1.0f;
    if (wd[MZ_DRQN_WDIR_M * E + e] > 0 && q.beta != 0.0) {
      const int j = (wd[MZ_DRQN_WDIR_B * E + e] + wd[MZ_DRQN_WDIR_K * E + e]) / q.T;
      const uint32_t mass = q.mem_prio[(size_t)wd[MZ_DRQN_WDIR_SLOT * E + e] * W + j];
      w = (float)pow((double)mmin / (double)mass, q.beta);
    }
    q.isw[e] = w;
  }
  if (tid == 0) {
    int64_t rows = 0, steps = 0;
    for (int e = 0; e < E; ++e) {
      const int m = wd[MZ_DRQN_WDIR_M * E + e];
      q.w_off[e] = rows;
      rows += m > 0 ? m + MZ_DRQN_WIN_PAD : 0;
      steps += m;
    }
    q.w_tot[0] = rows;
    q.w_tot[1] = steps;
  }
}

// one workgroup per learner, on its masses, directory block, seed, update count, burn-in and beta
__global__ __launch_bounds__(PRIO_T) void k_drqn_prio_sample(MzDrqnPopPrioSample q) {
  const int p = blockIdx.x;
  if (q.due && q.due[p] == 0) return;
  MzDrqnPrioSample s = q.s;
  const size_t E = (size_t)s.E;
  if (q.burn_in) s.K = drqn_pop_burn_in(q.burn_in, p, s.T, q.s.K);
  if (q.seed) s.seed = q.seed[p];
  if (q.counter) s.counter = q.counter[p];
  if (q.beta) s.beta = q.beta[p];
  s.mem_len += (size_t)p * s.cap;
  s.mem_prio += (size_t)p * s.cap * drqn_windows(s.L, s.T);
  s.mem_psum += (size_t)p * s.cap;
  s.wdir += (size_t)p * 5 * E;
  s.w_off += p * E;
  s.w_tot += 2 * (size_t)p;
  s.isw += p * E;
  drqn_prio_sample_body(s);
}

// the mass of a window whose residuals have the maximum mx and the mean `mean`:
// clamp(llrint((eta mx + (1 - eta) mean + eps)^alpha 2^20), 1, 2^30), 2^30 where that is not finite
__device__ __forceinline__ uint32_t drqn_prio_mass(const double mx, const double mean,
                                                   const double alpha, const double eta,
                                                   const double eps) {
  const double pr = __dadd_rn(__dmul_rn(eta, mx), __dmul_rn(1.0 - eta, mean));
  const double v = (alpha == 0.0 ? 1.0 : pow(pr + eps, alpha)) * (double)(1u << MZ_DRQN_PRIO_FRAC);
  if (!(v < (double)MZ_DRQN_PRIO_CEIL)) return MZ_DRQN_PRIO_CEIL;
  const long long r = llrint(v);
  return r < 1 ? 1u : (uint32_t)r;
}

// After the source forward, before the backward. A wave per window: lane i holds |qa - y| of
// training row i (T > 64: of rows i, i + 64, ...; the running maximum and the time-ordered
// float64 sum go round by round), lane 0 turns them into the mass, writes it to (slot, j) and
// raises prio_max (an integer atomic max); then the wave scales the window's d rows and its
// ep_loss by the importance weight. Once every mass of the batch is written, a wave per window
// recomputes its slot's sum from the slot's W entries (duplicates write the same values).
__device__ __forceinline__ void drqn_prio_update_body(const MzDrqnPrioUpdate& q) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int E = q.E, W = drqn_windows(q.L, q.T);
  const int64_t rows = (int64_t)E * (min(q.T, q.L) + MZ_DRQN_WIN_PAD);
  for (int pass = 0; pass < 2; ++pass) {
    for (int e = wave; e < E; e += PRIO_WAVES) {
      const int slot = q.wdir[MZ_DRQN_WDIR_SLOT * E + e], m = q.wdir[MZ_DRQN_WDIR_M * E + e];
      const int s = q.wdir[MZ_DRQN_WDIR_B * E + e] + q.wdir[MZ_DRQN_WDIR_K * E + e];
      const int64_t off = q.w_off[e];
      if (!(slot >= 0 && slot < q.cap && m >= 1 && m <= q.T && s >= 0 && s % q.T == 0 &&
            s / q.T < W && off >= 0 && off + m + MZ_DRQN_WIN_PAD <= rows))
        continue;
      uint32_t* pw = q.mem_prio + (size_t)slot * W;
      if (pass == 1) {
        uint64_t sum = 0;
        for (int j = lane; j < W; j += WAVE) sum += pw[j];
        sum = drqn_wave_scan(sum, lane);
        if (lane == WAVE - 1) q.mem_psum[slot] = sum;
        continue;
      }
      float mx = 0.0f;
      double sum = 0.0;
      for (int i0 = 0; i0 < m; i0 += WAVE) {
        const int64_t R = off + 1 + i0 + lane;
        const float a = i0 + lane < m ? fabsf(q.qa[R] - q.y[R]) : 0.0f;
        float v = a;
#pragma unroll
        for (int o = WAVE / 2; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
        mx = fmaxf(mx, v);
        const int cnt = min(WAVE, m - i0);
        for (int i = 0; i < cnt; ++i) sum += (double)__shfl(a, i);
      }
      if (lane == 0) {
        const uint32_t mass = drqn_prio_mass((double)mx, sum / (double)m, q.alpha, q.eta, q.eps);
        pw[s / q.T] = mass;
        atomicMax(q.prio_max, mass);
      }
      const float w = q.isw[e];
      for (int i = lane; i < m; i += WAVE) q.d[off + 1 + i] *= w;
      if (lane == 0) q.ep_loss[e] *= (double)w;
    }
    __threadfence_block();
    __syncthreads();
  }
}

// one workgroup per learner, with its alpha, eta and eps
__global__ __launch_bounds__(PRIO_T) void k_drqn_prio_update(MzDrqnPopPrioUpdate q) {
  const int p = blockIdx.x;
  if (q.due && q.due[p] == 0) return;
  MzDrqnPrioUpdate u = q.u;
  const size_t E = (size_t)u.E, rows = E * (min(u.T, u.L) + MZ_DRQN_WIN_PAD);
  if (q.alpha) u.alpha = q.alpha[p];
  if (q.eta) u.eta = q.eta[p];
  if (q.eps) u.eps = q.eps[p];
  u.wdir += p * 5 * E;
  u.w_off += p * E;
  u.w_tot += 2 * (size_t)p;
  u.qa += p * rows;
  u.y += p * rows;
  u.d += p * rows;
  u.ep_loss += p * E;
  u.isw += p * E;
  u.mem_prio += (size_t)p * u.cap * drqn_windows(u.L, u.T);
  u.mem_psum += (size_t)p * u.cap;
  u.prio_max += p;
  drqn_prio_update_body(u);
}

}  // namespace

hipError_t mz_launch_drqn_act(const MzDrqnPopAct& q, hipStream_t s) {
  const int bpl = (q.b + IPB - 1) / IPB;
  hipLaunchKernelGGL(k_drqn_act, dim3((unsigned)q.P * bpl), dim3(ACT_T), 0, s, q);
  return hipGetLastError();
}

hipError_t mz_launch_drqn_store(const MzDrqnPopStore& q, int blocks, hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_store, dim3(blocks, q.P), dim3(256), 0, s, q);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_drqn_ring, dim3((q.P + WAVE - 1) / WAVE), dim3(WAVE), 0, s, q);
  return hipGetLastError();
}

hipError_t mz_launch_drqn_sample(const MzDrqnPopSample& q, hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_sample, dim3(q.P), dim3(WAVE), (size_t)q.s.E * sizeof(int32_t), s, q);
  return hipGetLastError();
}

hipError_t mz_launch_drqn_seq_forward(const MzDrqnPopSeq& q, hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_seq_fwd, dim3((unsigned)q.P * q.q.u.E), dim3(WAVE), 0, s, q);
  return hipGetLastError();
}

hipError_t mz_launch_drqn_seq_backward(const MzDrqnPopSeq& q, hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_seq_bwd, dim3((unsigned)q.P * q.q.u.E), dim3(WAVE), 0, s, q);
  return hipGetLastError();
}

hipError_t mz_launch_drqn_reduce(const MzDrqnReduce& q, hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_reduce, dim3((MZ_DRQN_PARAMS + 255) / 256, q.P), dim3(256), 0, s, q);
  return hipGetLastError();
}

hipError_t mz_launch_drqn_pop_sync(const float* src, float* dst, const int32_t* mask, int P,
                                   hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_pop_sync, dim3((MZ_DRQN_PARAMS + 255) / 256, P), dim3(256), 0, s, src,
                     dst, mask);
  return hipGetLastError();
}

// ---- replay windows -------------------------------------------------------------------------
hipError_t mz_launch_drqn_snapshot(const MzDrqnSnap& q, hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_snapshot, dim3((q.B + 255) / 256, SNAP), dim3(256), 0, s, q);
  return hipGetLastError();
}

hipError_t mz_launch_drqn_snap_store(const MzDrqnPopSnapStore& q, int blocks, hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_snap_store, dim3(blocks, q.P), dim3(256), 0, s, q);
  return hipGetLastError();
}

hipError_t mz_launch_drqn_window_sample(const MzDrqnPopWinSample& q, hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_win_sample, dim3(q.P), dim3(WAVE), (size_t)q.w.s.E * sizeof(int32_t),
                     s, q);
  return hipGetLastError();
}

hipError_t mz_launch_drqn_window_forward(const MzDrqnPopWin& q, hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_win_fwd, dim3((unsigned)q.P * q.q.u.E), dim3(WAVE), 0, s, q);
  return hipGetLastError();
}

hipError_t mz_launch_drqn_window_backward(const MzDrqnPopWin& q, hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_win_bwd, dim3((unsigned)q.P * q.q.u.E), dim3(WAVE), 0, s, q);
  return hipGetLastError();
}

// ---- double-Q targets and n-step returns ----------------------------------------------------
hipError_t mz_launch_drqn_seq_forward_q(const MzDrqnPopSeqQ& q, hipStream_t s) {
  const dim3 grid((unsigned)q.q.P * q.q.q.u.E);
  if (q.q.q.u.target) hipLaunchKernelGGL(k_drqn_seq_fwd_q<FWD_Q4>, grid, dim3(WAVE), 0, s, q);
  else hipLaunchKernelGGL(k_drqn_seq_fwd_q<FWD_SEL>, grid, dim3(WAVE), 0, s, q);
  return hipGetLastError();
}

hipError_t mz_launch_drqn_window_forward_q(const MzDrqnPopWinQ& q, hipStream_t s) {
  const dim3 grid((unsigned)q.q.P * q.q.q.u.E);
  if (q.q.q.u.target) hipLaunchKernelGGL(k_drqn_win_fwd_q<FWD_Q4>, grid, dim3(WAVE), 0, s, q);
  else hipLaunchKernelGGL(k_drqn_win_fwd_q<FWD_SEL>, grid, dim3(WAVE), 0, s, q);
  return hipGetLastError();
}

hipError_t mz_launch_drqn_seq_returns(const MzDrqnPopSeqRet& q, hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_seq_ret, dim3((unsigned)q.q.P * q.q.q.u.E), dim3(WAVE), 0, s, q);
  return hipGetLastError();
}

hipError_t mz_launch_drqn_window_returns(const MzDrqnPopWinRet& q, hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_win_ret, dim3((unsigned)q.q.P * q.q.q.u.E), dim3(WAVE), 0, s, q);
  return hipGetLastError();
}

// ---- prioritized replay windows -------------------------------------------------------------
hipError_t mz_launch_drqn_prio_store(const MzDrqnPopPrioStore& q, int blocks, hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_prio_store, dim3(blocks, q.P), dim3(WAVE), 0, s, q);
  return hipGetLastError();
}

hipError_t mz_launch_drqn_prio_sample(const MzDrqnPopPrioSample& q, hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_prio_sample, dim3(q.P), dim3(PRIO_T), 0, s, q);
  return hipGetLastError();
}

hipError_t mz_launch_drqn_prio_update(const MzDrqnPopPrioUpdate& q, hipStream_t s) {
  hipLaunchKernelGGL(k_drqn_prio_update, dim3(q.P), dim3(PRIO_T), 0, s, q);
  return hipGetLastError();
}
