// mz_cae.hip — the convolutional autoencoder's decoder and reconstruction loss, f32, forward and
// backward, from the stem's features and the packed window bits.
//
// The reference pre-trains the conv stem as the encoder of an autoencoder
// (lib/models/convolutional_autoencoder.py, train_CAE.py): decoder ConvTranspose2d(32, 3, kernel 2,
// stride 2, output_padding 1) -> Sigmoid on the [32, 7, 7] stem output, loss
// alpha * MSE(Y, X) + (1 - alpha) * (1 - SSIM(Y, X)) with pytorch_msssim's defaults (11-tap
// Gaussian, sigma 1.5, valid filtering: 15x15 -> 5x5; C1 = 0.01^2, C2 = 0.03^2; mean of the map,
// no ReLU). The encoder is csrc/mz_stem.hip, unchanged; this file takes its feature rows and hands
// back dL/dfeat in the shape mz_stem_backward reads.
//
//   k_cae_decode   one workgroup per sample: Y = sigmoid(b[o] + sum_c feat[c,i,j] W[c,o,a,b]) at
//                  (2i+a, 2j+b); row / column 14 (the output padding) is sigmoid(b[o]);
//   k_cae_loss     one workgroup per sample, everything in LDS, Y never leaves the chip: decode,
//                  the target X unpacked from the bits (bit e of the sample = element e of
//                  [3][15][15]), F(Y), F(X), F(Y*Y), F(Y*X) (X is binary: F(X*X) = F(X)) filtered
//                  down the columns then along the rows, the 75 SSIM map entries and their
//                  derivatives, dL/dY through the transposed filters, dz = dY * y(1 - y), then
//                  dfeat (written to the gradient row), and this sample's terms of dW[32*3*2*2],
//                  db[3] and of the two loss sums into its row of the workspace;
//   k_cae_reduce   the per-sample rows summed in a fixed order (64 strided serial sums, then a
//                  fixed tree over them): dW, db, and loss3 = (loss, mse, ssim).
//
// Inputs, Y, dz, dfeat, dW and every output are f32. The SSIM stage between Y and dz runs in f64:
// the filters, the 75 map entries (sigma^2 = F(YY) - mu^2 cancels, and where the target is
// constant under a footprint the denominator is sigma1^2 + C2 alone, so f32 there costs up to
// 1e-5 of a gradient), their derivatives and the transposed filters. So do the sums of terms of
// both signs or of many samples that feed a handful of numbers: the squared-error and map sums
// and db, which cross the workspace as (hi, lo) f32 pairs. No atomics: identical calls, identical
// bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mz_learner.h"

namespace {

constexpr int FEAT = 1568;  // 32 x 7 x 7
constexpr int NPOOL = 49;
constexpr int WW = 22;      // window words per sample
constexpr int NE = 675;     // 3 x 15 x 15
constexpr int NW = 384;     // 32 x 3 x 2 x 2
constexpr int NM = 75;      // 3 x 5 x 5 SSIM map entries per sample
// workspace floats per sample: dW[384] | db[3] as hi lo pairs, one zero pair | sse hi lo | ssim hi lo
constexpr int ROW = 396;
constexpr int DB_AT = 384, SSE_AT = 392, SSIM_AT = 394;
constexpr int NT = 256;

struct Gauss { double g[11]; };

__device__ inline float sigmoidf_(float z) { return 1.0f / (1.0f + expf(-z)); }

// feat row, decoder weights and bias -> LDS
__device__ inline void load_params(const float* __restrict__ feat, const float* __restrict__ w,
                                   const float* __restrict__ b, float* fs, float* wsm, float* bs) {
  const int tid = threadIdx.x;
  for (int i = tid; i < FEAT; i += NT) fs[i] = feat[i];
  for (int i = tid; i < NW; i += NT) wsm[i] = w[i];
  if (tid < 3) bs[tid] = b[tid];
}

// element e = o*225 + r*15 + c of Y
__device__ inline float decode_at(int e, const float* fs, const float* wsm, const float* bs) {
  const int o = e / 225, rc = e - o * 225, r = rc / 15, c = rc - r * 15;
  float z = bs[o];
  if (r < 14 && c < 14) {
    const float* f = fs + (r >> 1) * 7 + (c >> 1);
    const float* wk = wsm + o * 4 + (r & 1) * 2 + (c & 1);
#pragma unroll 8
    for (int k = 0; k < 32; ++k) z = fmaf(f[k * NPOOL], wk[k * 12], z);
  }
  return sigmoidf_(z);
}

__global__ __launch_bounds__(NT) void k_cae_decode(const float* __restrict__ feat, int ld, int n,
                                                   const float* __restrict__ w,
                                                   const float* __restrict__ b,
                                                   float* __restrict__ out) {
  __shared__ float fs[FEAT];
  __shared__ float wsm[NW];
  __shared__ float bs[4];
  const int s = blockIdx.x;
  if (s >= n) return;
  load_params(feat + (size_t)s * ld, w, b, fs, wsm, bs);
  __syncthreads();
  for (int e = threadIdx.x; e < NE; e += NT) out[(size_t)s * NE + e] = decode_at(e, fs, wsm, bs);
}

// sum of one double per thread over the workgroup, fixed order; valid in thread 0
__device__ inline double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  const int tid = threadIdx.x;
  __syncthreads();  // red free
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(NT) void k_cae_loss(const uint32_t* __restrict__ bits,
                                                 const float* __restrict__ feat, int ld, int n,
                                                 const float* __restrict__ w,
                                                 const float* __restrict__ b, Gauss gk,
                                                 double cmse, double cssim,
                                                 float* __restrict__ gfeat, int ldg, int grad,
                                                 float* __restrict__ ws) {
  __shared__ float fs[FEAT];
  __shared__ float wsm[NW];
  __shared__ float bs[4];
  __shared__ uint32_t wb[WW];
  __shared__ float Ys[NE], Xs[NE];
  __shared__ double T1[4 * 225];  // [q][ch][i < 5][c < 15]
  __shared__ double Ms[4 * NM];   // [q][ch][i][j]: F(Y), F(X), F(YY), F(YX)
  __shared__ double Gs[3 * NM];   // dL/dmu1, dL/dF(YY), dL/dF(YX)
  __shared__ double Us[3 * 225];  // [q][ch][i < 5][c < 15]
  __shared__ float dz[NE];
  __shared__ double gs[11];
  __shared__ double red[4];
  const int tid = threadIdx.x, s = blockIdx.x;
  if (s >= n) return;
  load_params(feat + (size_t)s * ld, w, b, fs, wsm, bs);
  if (tid < WW) wb[tid] = bits[(size_t)s * WW + tid];
  if (tid < 11) gs[tid] = gk.g[tid];
  __syncthreads();
  double sse = 0.0;
  for (int e = tid; e < NE; e += NT) {
    const float y = decode_at(e, fs, wsm, bs);
    const float x = (float)((wb[e >> 5] >> (e & 31)) & 1u);
    Ys[e] = y;
    Xs[e] = x;
    const double d = (double)y - (double)x;
    sse += d * d;
  }
  __syncthreads();
  // filter down the columns: T1[q][ch][i][c] = sum_k g[k] v_q[ch][i + k][c]
  for (int t = tid; t < 4 * 225; t += NT) {
    const int q = t / 225, r = t - q * 225, ch = r / 75, ic = r - ch * 75, i = ic / 15,
              c = ic - i * 15;
    const int base = ch * 225 + i * 15 + c;
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const double y = Ys[base + 15 * k], x = Xs[base + 15 * k];
      const double v = q == 0 ? y : q == 1 ? x : q == 2 ? y * y : y * x;
      a = fma(gs[k], v, a);
    }
    T1[t] = a;
  }
  __syncthreads();
  // then along the rows: Ms[q][ch][i][j] = sum_k g[k] T1[q][ch][i][j + k]
  for (int t = tid; t < 4 * NM; t += NT) {
    const int qc = t / 25, ij = t - qc * 25, i = ij / 5, j = ij - i * 5;
    const double* p = T1 + qc * 75 + i * 15 + j;
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < 11; ++k) a = fma(gs[k], p[k], a);
    Ms[t] = a;
  }
  __syncthreads();
  double smap = 0.0;
  if (tid < NM) {
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    const double m1 = Ms[tid], m2 = Ms[NM + tid], fyy = Ms[2 * NM + tid], fyx = Ms[3 * NM + tid];
    const double s1 = fyy - m1 * m1, s2 = m2 - m2 * m2, s12 = fyx - m1 * m2;
    const double A1 = 2.0 * m1 * m2 + C1, B1 = m1 * m1 + m2 * m2 + C1;
    const double A2 = 2.0 * s12 + C2, B2 = s1 + s2 + C2;
    const double l = A1 / B1, cs = A2 / B2;
    smap = l * cs;
    // d map / d F(YX), d F(YY), d mu1 (sigma12 = F(YX) - mu1 mu2, sigma1^2 = F(YY) - mu1^2),
    // times dL/dmap = -(1 - alpha) / (75 n)
    const double dfyx = 2.0 * l / B2;
    const double dfyy = -(l * cs) / B2;
    const double dm1 = cs * (2.0 * m2 - 2.0 * m1 * l) / B1 + l * (2.0 * m1 * cs - 2.0 * m2) / B2;
    Gs[tid] = cssim * dm1;
    Gs[NM + tid] = cssim * dfyy;
    Gs[2 * NM + tid] = cssim * dfyx;
  }
  const double sse_all = block_sum(sse, red);
  const double smap_all = block_sum(smap, red);
  float* row = ws + (size_t)s * ROW;
  if (tid == 0) {
    const float h0 = (float)sse_all, h1 = (float)smap_all;
    row[SSE_AT] = h0;
    row[SSE_AT + 1] = (float)(sse_all - (double)h0);
    row[SSIM_AT] = h1;
    row[SSIM_AT + 1] = (float)(smap_all - (double)h1);
    row[DB_AT + 6] = 0.0f;  // the unused pair of the db block
    row[DB_AT + 7] = 0.0f;
  }
  if (!grad) return;
  __syncthreads();
  // transposed filters, rows first: Us[q][ch][i][c] = sum_j g[c - j] G_q[ch][i][j]
  for (int t = tid; t < 3 * 225; t += NT) {
    const int qc = t / 75, ic = t - qc * 75, i = ic / 15, c = ic - i * 15;
    const double* p = Gs + qc * 25 + i * 5;
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int k = c - j;
      if (k >= 0 && k <= 10) a = fma(gs[k], p[j], a);
    }
    Us[t] = a;
  }
  __syncthreads();
  // then columns, the MSE term and the sigmoid: dz (f32, rounded once)
  for (int e = tid; e < NE; e += NT) {
    const int ch = e / 225, rc = e - ch * 225, r = rc / 15, c = rc - r * 15;
    double v[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double* p = Us + (q * 3 + ch) * 75 + c;
      double a = 0.0;
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int k = r - i;
        if (k >= 0 && k <= 10) a = fma(gs[k], p[15 * i], a);
      }
      v[q] = a;
    }
    const double y = Ys[e], x = Xs[e];
    const double dy = (cmse * (y - x) + v[0]) + (2.0 * y * v[1] + x * v[2]);
    dz[e] = (float)(dy * (y * (1.0 - y)));  // y == 0 or 1 exactly: 0
  }
  __syncthreads();
  if (gfeat) {  // dfeat[c][i][j] = sum_{o,a,b} dz[o][2i+a][2j+b] W[c][o][a][b]
    float* gr = gfeat + (size_t)s * ldg;
    for (int f = tid; f < FEAT; f += NT) {
      const int c = f / NPOOL, q = f - c * NPOOL, i = q / 7, j = q - i * 7;
      const float* d0 = dz + 30 * i + 2 * j;
      const float* wk = wsm + c * 12;
      float a = 0.0f;
#pragma unroll
      for (int o = 0; o < 3; ++o) {
        a = fmaf(d0[o * 225], wk[o * 4], a);
        a = fmaf(d0[o * 225 + 1], wk[o * 4 + 1], a);
        a = fmaf(d0[o * 225 + 15], wk[o * 4 + 2], a);
        a = fmaf(d0[o * 225 + 16], wk[o * 4 + 3], a);
      }
      gr[f] = a;
    }
  }
  // this sample's dW[c][o][a][b] = sum_{i,j} feat[c][i][j] dz[o][2i+a][2j+b]
  for (int t = tid; t < NW; t += NT) {
    const int c = t / 12, k = t - c * 12, o = k >> 2, ab = k & 3;
    const float* d0 = dz + o * 225 + (ab >> 1) * 15 + (ab & 1);
    const float* f = fs + c * NPOOL;
    float a = 0.0f;
    for (int i = 0; i < 7; ++i)
#pragma unroll
      for (int j = 0; j < 7; ++j) a = fmaf(f[i * 7 + j], d0[30 * i + 2 * j], a);
    row[t] = a;
  }
  // db[o]: wave o sums channel o's 225 entries (terms of both signs: in f64, as a hi / lo pair)
  const int lane = tid & 63, wv = tid >> 6;
  if (wv < 3) {
    double a = 0.0;
    for (int i = lane; i < 225; i += 64) a += (double)dz[wv * 225 + i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o);
    if (lane == 0) {
      const float h = (float)a;
      row[DB_AT + 2 * wv] = h;
      row[DB_AT + 2 * wv + 1] = (float)(a - (double)h);
    }
  }
}

// Column k of block blockIdx.x's four: thread (sl = tid >> 2, k = tid & 3) sums samples sl,
// sl + 64, ... in order, then a fixed tree over sl. Blocks below NW / 4 sum the dW columns in f32;
// the last three sum hi / lo pairs in f64 (two pairs per block): db[0..2] and the two loss sums,
// whose block writes loss3.
__global__ __launch_bounds__(NT) void k_cae_reduce(const float* __restrict__ ws, int n,
                                                   float alpha, float* __restrict__ dw,
                                                   float* __restrict__ db,
                                                   float* __restrict__ loss3) {
  __shared__ double redd[NT];
  __shared__ float redf[NT];
  const int tid = threadIdx.x, sl = tid >> 2, k = tid & 3;
  const int col = blockIdx.x * 4 + k;
  if (col - k >= DB_AT) {
    const bool losses = col - k == SSE_AT;
    if (!losses && !db) return;  // uniform
    double a = 0.0;
    if (k < 2) {
      const float* p = ws + (col - k) + 2 * k;
      for (int s = sl; s < n; s += 64) a += (double)p[(size_t)s * ROW] + (double)p[(size_t)s * ROW + 1];
    }
    redd[tid] = a;
    __syncthreads();
    for (int h = 32; h >= 1; h >>= 1) {
      if (sl < h) redd[tid] += redd[tid + 4 * h];
      __syncthreads();
    }
    if (losses) {
      if (tid == 0) {
        const double mse = redd[0] / (675.0 * (double)n), ssim = redd[1] / (75.0 * (double)n);
        const double al = (double)alpha;
        loss3[0] = (float)(al * mse + (1.0 - al) * (1.0 - ssim));
        loss3[1] = (float)mse;
        loss3[2] = (float)ssim;
      }
    } else if (tid < 2) {
      const int o = (col - k - DB_AT) / 2 + tid;
      if (o < 3) db[o] = (float)redd[tid];
    }
    return;
  }
  if (!dw) return;  // uniform: a forward-only call
  float a = 0.0f;
  const float* p = ws + col;
  int s = sl;
  for (; s + 64 * 7 < n; s += 64 * 8) {  // 8 loads in flight, summed in the same order
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(s + 64 * u) * ROW];
#pragma unroll
    for (int u = 0; u < 8; ++u) a += v[u];
  }
  for (; s < n; s += 64) a += p[(size_t)s * ROW];
  redf[tid] = a;
  __syncthreads();
  for (int h = 32; h >= 1; h >>= 1) {
    if (sl < h) redf[tid] += redf[tid + 4 * h];
    __syncthreads();
  }
  if (tid < 4) dw[col] = redf[tid];
}

Gauss gauss_window() {
  Gauss gk;
  double sum = 0.0;
  for (int k = 0; k < 11; ++k) {
    gk.g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
    sum += gk.g[k];
  }
  for (int k = 0; k < 11; ++k) gk.g[k] /= sum;
  return gk;
}

}  // namespace

int mz_cae_ws_floats(int n) { return n > 0 ? n * ROW : 0; }

hipError_t mz_launch_cae_decode(const float* feat, int ld, int n, const float* w, const float* b,
                                float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_cae_decode, dim3(n), dim3(NT), 0, s, feat, ld, n, w, b, out);
  return hipGetLastError();
}

hipError_t mz_launch_cae_loss(const uint32_t* bits, const float* feat, int ld, int n, const float* w,
                              const float* b, float alpha, float* loss3, float* gfeat, int ldg,
                              float* dw, float* db, float* ws, hipStream_t s) {
  static const Gauss gk = gauss_window();
  // dL/dY's MSE factor 2 alpha / (675 n) and dL/dmap = -(1 - alpha) / (75 n)
  const double cmse = 2.0 * (double)alpha / (675.0 * (double)n);
  const double cssim = -(1.0 - (double)alpha) / (75.0 * (double)n);
  const int grad = (gfeat || dw || db) ? 1 : 0;
  hipLaunchKernelGGL(k_cae_loss, dim3(n), dim3(NT), 0, s, bits, feat, ld, n, w, b, gk, cmse, cssim,
                     gfeat, ldg, grad, ws);
  // without dW / db only the block of the loss sums has work; every column read was written
  hipLaunchKernelGGL(k_cae_reduce, dim3(ROW / 4), dim3(NT), 0, s, ws, n, alpha, dw, db, loss3);
  return hipGetLastError();
}
