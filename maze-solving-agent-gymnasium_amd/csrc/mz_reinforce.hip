// mz_reinforce.hip — REINFORCE's own arithmetic on the device: the temperature draw, the
// per-episode return normalisation, and the policy-gradient + entropy loss with its gradient.
//
// Reference (one env): RFAgent (agents/rf_agent.py:51-129) driven by ValueBasedTrainer.train
// (lib/trainers/value_based_trainer.py:25-92): select_action (:73-86: softmax(logits / 2),
// torch.multinomial, log(p + 1e-10) of the draw and of all four entries) per step; at the
// episode's end get_returns (:88-99: R = r + gamma R backwards over Python floats, float32,
// (R - mean) / (std + 1e-6) with the unbiased std) and optimize_model (:101-126: adv = R - mean(R),
// loss = sum_t -log_prob_t adv_t - 0.01 mean_t(-sum_k l_tk exp(l_tk)), clip_grad_norm_(1), AdamW).
//
// Vectorised (trainers/reinforce_trainer.py VectorReinforceTrainer): the [B][L] episode records,
// k_ppo_scan and the update pool are PPO's (mz_ppo.hip). Per vector step:
//   k_rf_act     the draw from softmax(logits / tau) (torch's 4-wide softmax, inverse CDF of a
//                Philox uniform) and the record of (obs6, window bits, action) at t[i]. No
//                log-prob and no value are recorded: the update recomputes the forward;
//   (mz_step, k_ppo_scan)
//   k_rf_finish  one workgroup per finished episode: get_returns and the second mean
//                subtraction, and the episode's rows (with its length on every row) appended to
//                the pool; the pooled-episode counter.
// At an update, per chunk of pool rows:
//   k_rf_head    f = (1/E)(-adv l_a - (coef / T)(-sum_k q_k l_k)), q = softmax(x / tau) + 1e-10,
//                l = log q, per row; the chunk's sum (float64, fixed order) and d f / d logits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mz_common.h"
#include "mz_learner.h"

namespace {

constexpr int WAVE = 64;
constexpr int ACT_IPB = 8;    // instances per k_rf_act workgroup (32 lanes each)
constexpr int FIN_T = 256;    // k_rf_finish threads per episode
constexpr int FIN_CH = 2048;  // rewards staged in LDS per chunk of the serial returns pass
constexpr int HEAD_T = 1024;  // k_rf_head threads (one workgroup)

__global__ __launch_bounds__(32 * ACT_IPB) void k_rf_act(MzRfAct q) {
  const int slot = threadIdx.x >> 5, w = threadIdx.x & 31;
  const int i = blockIdx.x * ACT_IPB + slot;
  if (i >= q.B) return;
  const int t = q.t[i];
  const bool rec = t >= 0 && t < q.L;  // never outside the episode buffers; the draw happens anyway
  const size_t row = rec ? (size_t)i * q.L + t : 0;
  if (w < 6) {
    if (rec) q.b_s6[row * 6 + w] = q.obs6[(size_t)i * 6 + w];
  } else if (w < 28) {
    if (rec) q.b_w[row * 22 + (w - 6)] = q.bits[(size_t)i * 22 + (w - 6)];
  } else if (w == 28) {
    // softmax(logits / tau) as torch's kernel forms it for a 4-wide row: max and sum by
    // xor-butterfly over a 4-lane group, exp(x - max) / sum
    float x[4], e[4], p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = __fdiv_rn(q.logits[(size_t)i * q.ldl + k], q.tau);
    const float m = fmaxf(fmaxf(x[0], x[2]), fmaxf(x[1], x[3]));
#pragma unroll
    for (int k = 0; k < 4; ++k) e[k] = expf(x[k] - m);
    const float s = (e[0] + e[2]) + (e[1] + e[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = e[k] / s;
    uint32_t u[4];
    mz_philox(q.seed, MZ_RF_STREAM ^ ((uint64_t)(uint32_t)i << 32), q.counter, u);
    const float r = (float)(u[0] >> 8) * (1.0f / 16777216.0f);  // [0, 1), 24 bits
    // inverse CDF; the last entry with nonzero probability if rounding leaves r above the sum
    int a = -1;
    float c = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      c += p[k];
      if (a < 0 && r < c) a = k;
    }
    if (a < 0)
      for (int k = 3; k >= 0; --k)
        if (p[k] > 0.0f) { a = k; break; }
    if (a < 0) a = 0;  // all-NaN logits: torch would raise; act 0 (the loss goes NaN anyway)
    if (rec) q.b_a[row] = a;
    q.act_out[i] = a;
  }
}

__device__ inline double block_sum(double v, double* red) {
  for (int o = WAVE / 2; o; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  double s = 0.0;
  for (int k = 0; k < FIN_T / WAVE; ++k) s += red[k];  // same order in every thread
  return s;
}

__global__ __launch_bounds__(FIN_T) void k_rf_finish(MzRfFinish q) {
  __shared__ double rbuf[FIN_CH];
  __shared__ float fbuf[FIN_CH];
  __shared__ double red[FIN_T / WAVE];
  const int nfin = *q.fin_count < q.B ? *q.fin_count : q.B;  // the lists hold B entries
  for (int k = blockIdx.x; k < nfin; k += gridDim.x) {
    const int i = q.fin_id[k];
    const int n = q.fin_len[k];
    const int64_t o = q.fin_off[k];
    // overflow: nothing written (the host sees fill > capacity); a listed episode is inside the
    // record buffers by k_ppo_scan's construction, checked again here
    if (o < 0 || o + n > q.cap || i < 0 || i >= q.B || n < 1 || n > q.L) continue;
    const double* r = q.b_r + (size_t)i * q.L;
    float* adv = q.p_adv + o;
    // 1. returns, backwards in float64 (R = r + gamma R), stored as float32; chunks of FIN_CH
    //    rewards staged in LDS, the recurrence run by thread 0
    double acc = 0.0, sum = 0.0;
    for (int end = n; end > 0; end -= FIN_CH) {
      const int beg = end > FIN_CH ? end - FIN_CH : 0;
      __syncthreads();
      for (int t = beg + threadIdx.x; t < end; t += FIN_T) rbuf[t - beg] = r[t];
      __syncthreads();
      if (threadIdx.x == 0) {
        for (int t = end - 1; t >= beg; --t) {
          acc = __dadd_rn(rbuf[t - beg], __dmul_rn(q.gamma, acc));
          fbuf[t - beg] = (float)acc;
        }
      }
      __syncthreads();
      for (int t = beg + threadIdx.x; t < end; t += FIN_T) {
        const float x = fbuf[t - beg];
        adv[t] = x;
        sum += (double)x;
      }
    }
    __syncthreads();  // adv[] written by this workgroup, read back below
    // 2. (R - mean) / (std + 1e-6), unbiased std (torch.std): sums in float64, mean / std
    //    rounded to f32
    const double mean = block_sum(sum, red) / n;
    double ss = 0.0;
    for (int t = threadIdx.x; t < n; t += FIN_T) {
      const double d = (double)adv[t] - mean;
      ss += d * d;
    }
    const float m32 = (float)mean;
    const float s32 = __fadd_rn((float)sqrt(block_sum(ss, red) / (n - 1)), 1e-6f);
    double asum = 0.0;
    for (int t = threadIdx.x; t < n; t += FIN_T) {
      const float rn = __fdiv_rn(__fsub_rn(adv[t], m32), s32);
      adv[t] = rn;
      asum += (double)rn;
    }
    // 3. optimize_model's baseline: adv = R - mean(R) (each thread re-reads its own rows)
    const float am32 = (float)(block_sum(asum, red) / n);
    for (int t = threadIdx.x; t < n; t += FIN_T) adv[t] = __fsub_rn(adv[t], am32);
    // 4. the episode's states, actions and length into the pool rows
    const size_t src = (size_t)i * q.L;
    for (int t = threadIdx.x; t < n; t += FIN_T) {
      q.p_a[o + t] = q.b_a[src + t];
      q.p_len[o + t] = n;
    }
    for (int e = threadIdx.x; e < n * 6; e += FIN_T) q.p_s6[o * 6 + e] = q.b_s6[src * 6 + e];
    for (int e = threadIdx.x; e < n * 22; e += FIN_T) q.p_w[o * 22 + e] = q.b_w[src * 22 + e];
    if (threadIdx.x == 0) atomicAdd(q.episodes, 1);  // integer: the order does not matter
  }
}

// One workgroup: per row the loss term and d f / d logits, then the chunk's sum by a fixed tree.
// The row arithmetic runs in float64 from the f32 logits (four exp and four log per row): with
// p_a near 1, g_a - sum_k p_k g_k cancels to (1 - p_a), and the +1e-10 decides rows whose drawn
// action has p < 1e-10.
__global__ __launch_bounds__(HEAD_T) void k_rf_head(MzRfHead q) {
  __shared__ double red[HEAD_T];
  const int tid = threadIdx.x;
  const double inv_e = 1.0 / (double)*q.episodes;
  const double tau = (double)q.tau, coef = (double)q.coef;
  double acc = 0.0;
  for (int i = tid; i < q.b; i += HEAD_T) {
    const float* x = q.logits + (size_t)i * q.ldl;
    double z[4], p[4], l[4], g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = (double)x[k] / tau;
    const double m = fmax(fmax(z[0], z[2]), fmax(z[1], z[3]));
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      p[k] = exp(z[k] - m);
      s += p[k];
    }
    const int a = (int)q.action[i];
    const double adv = (double)q.adv[i];
    const double ct = coef / (double)q.len[i];
    double la = 0.0, ent = 0.0, pg = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      p[k] /= s;
      const double qk = p[k] + 1e-10;
      l[k] = log(qk);
      ent -= qk * l[k];
      g[k] = ct * (l[k] + 1.0);
      if (k == a) {  // (selects: a dynamic index would move the arrays out of registers)
        la = l[k];
        g[k] -= adv / qk;
      }
      g[k] *= inv_e;
      pg += p[k] * g[k];
    }
    acc += inv_e * (-adv * la - ct * ent);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      q.dlogits[(size_t)i * q.ldg + k] = (float)(p[k] * (g[k] - pg) / tau);
  }
  red[tid] = acc;
  __syncthreads();
  for (int o = HEAD_T / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) *q.loss = (float)red[0];
}

}  // namespace

hipError_t mz_launch_rf_act(const MzRfAct& q, hipStream_t s) {
  if (q.B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rf_act, dim3((q.B + ACT_IPB - 1) / ACT_IPB), dim3(32 * ACT_IPB), 0, s, q);
  return hipGetLastError();
}

hipError_t mz_launch_rf_finish(const MzRfFinish& q, hipStream_t s) {
  if (q.B <= 0) return hipSuccess;
  const int blocks = q.B < 2048 ? q.B : 2048;
  hipLaunchKernelGGL(k_rf_finish, dim3(blocks), dim3(FIN_T), 0, s, q);
  return hipGetLastError();
}

hipError_t mz_launch_rf_head(const MzRfHead& q, hipStream_t s) {
  if (q.b <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rf_head, dim3(1), dim3(HEAD_T), 0, s, q);
  return hipGetLastError();
}
