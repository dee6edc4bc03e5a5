// mz_learner.h — launchers of the learner / trainer kernels (mz_stem, mz_optim, mz_qnet,
// mz_trainer, mz_ppo, mz_reinforce, mz_drqn, mz_qact), used by the C ABI (mz_api.hip).
#pragma once
#include "mz_kernels.h"

int mz_stem_chunks(int n);
hipError_t mz_launch_stem_fwd(const uint32_t* bits, const float* obs6, int n, const float* w,
                              const float* b, float drop_p, const uint64_t* rng, uint32_t salt,
                              float* feat, int ld, uint8_t* code, hipStream_t s);
hipError_t mz_launch_stem_bwd(const uint32_t* bits, const uint8_t* code, const float* g, int ld,
                              int n, float drop_p, float* partial, float* dw, float* db,
                              hipStream_t s, uint64_t* advance = nullptr);
// ---- the autoencoder's decoder + reconstruction loss (mz_cae.hip)
#define MZ_CAE_MAX_N (1 << 22)  // samples per call (the workspace size stays an int)
int mz_cae_ws_floats(int n);
hipError_t mz_launch_cae_decode(const float* feat, int ld, int n, const float* w, const float* b,
                                float* out, hipStream_t s);
hipError_t mz_launch_cae_loss(const uint32_t* bits, const float* feat, int ld, int n, const float* w,
                              const float* b, float alpha, float* loss3, float* gfeat, int ldg,
                              float* dw, float* db, float* ws, hipStream_t s);
#define MZ_OPT_MAX_SEGS 16

hipError_t mz_launch_adamw(float* p, float* m, float* v, const float* const* grads,
                           const int64_t* seg_len, int nseg, const float* lr, float* step, double b1,
                           double b2, double eps, double wd, float clamp, float gscale,
                           int write_grad, hipStream_t s);
hipError_t mz_launch_pair_surrogate(const float* lp_new, const float* lp_old, const float* adv,
                                    int b, float clip, float* part, float* dsum, hipStream_t s);
hipError_t mz_launch_leaky_bf16(uint16_t* x, int64_t n, float slope, hipStream_t s);
hipError_t mz_launch_colsum(const float* g, int n, int m, int ld, float* out, hipStream_t s);
hipError_t mz_launch_replay_gather(const int64_t* idx, int b, int64_t cap, const float* s6,
                                   const uint32_t* sw, const int64_t* a, const float* r,
                                   const float* s6n, const uint32_t* swn, float* o6, uint32_t* ow,
                                   int64_t* oa, float* orw, hipStream_t s);

// ---- trainer bookkeeping (mz_trainer.hip)
struct MzHeadBf16 {  // acting head: f32 Linear weights / biases -> bf16 (fc1 permuted + padded)
  const float* w[3];
  const float* b[3];
  uint16_t* dw[3];
  uint16_t* db[3];
  int out[3], in[3];
  int ld0, conv_out, conv_ch;
};
struct MzReplayPush {  // ring rows ptr .. ptr + n - 1 <- n source rows, per array (NULL src: skip)
  const void* src[6];  // obs6, bits, action (int32 -> int64), reward, next obs6, next bits
  void* dst[6];
  int words[6];        // 32-bit words per row
  int n;
  int64_t cap, ptr;
};
hipError_t mz_launch_greedy_list(const MzAct& ap, int n, const int32_t* blk, int32_t* rows,
                                 int32_t* count, int32_t* count_host, hipStream_t s);
hipError_t mz_launch_tick(const uint8_t* term, const uint8_t* trunc, float* steps_done,
                          float eps_final, float eps_span, float inv_decay, float* eps_out,
                          unsigned long long* wins, unsigned long long* episodes, uint64_t seed,
                          uint64_t counter, int n, int32_t* scratch, int32_t* rows, int32_t* count,
                          hipStream_t s);
hipError_t mz_launch_greedy_scatter(const uint16_t* q, int ldq, const int32_t* rows,
                                    const int32_t* count, int m, int64_t* greedy, hipStream_t s);
hipError_t mz_launch_head_bf16(const MzHeadBf16& h, hipStream_t s);
hipError_t mz_launch_replay_push(const MzReplayPush& p, hipStream_t s);
hipError_t mz_launch_replay_idx(uint64_t seed, uint64_t counter, int64_t newest, int64_t n_avail,
                                int64_t cap, int64_t* out, int n, hipStream_t s);
hipError_t mz_launch_q_loss(const float* q, int ldq, const float* qn, int ldn, const float* qt,
                            int ldt, const int64_t* action, const float* reward, float gamma, int b,
                            float* loss, float* diff, hipStream_t s);
hipError_t mz_launch_q_loss_bwd(const float* g, const float* diff, const int64_t* action, int b,
                                int rows, float norm, float* dq, hipStream_t s);
// the Q head (act(z2) -> fc3) of the source's and the target's rows + the loss (mz_trainer.hip)
struct MzHeadLoss {
  const float *z2s, *w3s, *b3s, *z2t, *w3t, *b3t;
  int lds, ldt, dbl, b, H, act;
  const int64_t* action;
  const float* reward;
  float gamma;
  float* part;      // [mz_head_loss_blocks(b)]
  unsigned* ticket; // unused since round 5 (the partials are summed by a second launch)
  float *loss, *diff;
};
int mz_head_loss_blocks(int b);
int mz_head_loss_bwd_blocks(int b);
hipError_t mz_launch_head_loss(const MzHeadLoss& p, hipStream_t s);
hipError_t mz_launch_head_loss_bwd(const float* g, const float* diff, const int64_t* action, int b,
                                   float norm, const float* z2s, int lds, const float* w3s, int H,
                                   int act, float* dz2, int ldd, float* part, hipStream_t s);
hipError_t mz_launch_adamw_groups(float* p, float* m, float* v, const float* const* grads,
                                  const int64_t* seg_len, const int32_t* seg_group, int nseg,
                                  const float* lr, float* step, double b1, double b2, double eps,
                                  double wd, float max_norm, float* scratch, hipStream_t s);

// ---- PPO rollout (mz_ppo.hip) ------------------------------------------------------------
struct MzPpoAct {
  const float* logits; int ldl;     // actor logits [B][ldl >= 4], f32
  const float* value; int ldv;      // critic values [B] (stride ldv)
  const float* obs6; const uint32_t* bits;
  int B, L;                         // instances, episode buffer length
  uint64_t seed, counter;
  const int32_t* t;                 // per-instance step index
  float* b_s6; uint32_t* b_w; int64_t* b_a; float* b_lp; float* b_v;  // [B][L] records
  int32_t* act_out;                 // [B] actions for mz_step
};
struct MzPpoScan {
  const double* reward64; const uint8_t* term; const uint8_t* trunc;
  int B, L;
  int32_t* t; double* b_r;
  int32_t* fin_id; int64_t* fin_off; int32_t* fin_len; int32_t* fin_count;
  int64_t* pool_fill; int64_t* pool_total; long long* stats;
};
struct MzPpoFinish {
  const double* b_r; const float* b_s6; const uint32_t* b_w; const int64_t* b_a; const float* b_lp;
  const float* b_v; int L;
  const int32_t* fin_id; const int64_t* fin_off; const int32_t* fin_len; const int32_t* fin_count;
  double gamma; int64_t cap;
  float* p_s6; uint32_t* p_w; int64_t* p_a; float* p_lp; float* p_adv; float* p_ret;
};
hipError_t mz_launch_ppo_act(const MzPpoAct& q, hipStream_t s);
hipError_t mz_launch_ppo_scan(const MzPpoScan& q, hipStream_t s);
hipError_t mz_launch_ppo_finish(const MzPpoFinish& q, int max_episodes, hipStream_t s);
struct MzPpoHead {  // fused loss of one minibatch (4 actions)
  const float* logits; int ldl; const float* value; int ldv;
  const int64_t* action; const float* lp_old; const float* adv; const float* ret;
  const float* coef; int b;
  float* lp_new; float* ent; float* p; float* dent; float* part; float* dsum;  // scratch
  float* loss; float* dlogits; int ldg; float* dvalue; int ldvg;
};
hipError_t mz_launch_ppo_head(const MzPpoHead& q, float clip, hipStream_t s);

// ---- REINFORCE (mz_reinforce.hip); the records, k_ppo_scan and the pool are PPO's -------------
struct MzRfAct {
  const float* logits; int ldl; float tau;  // policy logits [B][ldl >= 4], f32; temperature
  const float* obs6; const uint32_t* bits;
  int B, L;
  uint64_t seed, counter;
  const int32_t* t;
  float* b_s6; uint32_t* b_w; int64_t* b_a;  // [B][L] records
  int32_t* act_out;
};
struct MzRfFinish {
  const double* b_r; const float* b_s6; const uint32_t* b_w; const int64_t* b_a; int B, L;
  const int32_t* fin_id; const int64_t* fin_off; const int32_t* fin_len; const int32_t* fin_count;
  double gamma; int64_t cap;
  float* p_s6; uint32_t* p_w; int64_t* p_a; float* p_adv; int32_t* p_len;
  int32_t* episodes;                         // += the episodes pooled
};
struct MzRfHead {
  const float* logits; int ldl;
  const int64_t* action; const float* adv; const int32_t* len; const int32_t* episodes;
  int b; float tau, coef;
  float* loss; float* dlogits; int ldg;
};
hipError_t mz_launch_rf_act(const MzRfAct& q, hipStream_t s);
hipError_t mz_launch_rf_finish(const MzRfFinish& q, hipStream_t s);
hipError_t mz_launch_rf_head(const MzRfHead& q, hipStream_t s);

// ---- recurrent DQN (mz_drqn.hip); the reward records and k_ppo_scan are PPO's ------------------
#define MZ_DRQN_HIDDEN 32
#define MZ_DRQN_PARAMS 5252     // 128 x 6 + 128 x 32 + 128 + 128 + 4 x 32 + 4
#define MZ_DRQN_ROW_WORDS 8     // a replay row: x[6] f32, action i32, reward f32
#define MZ_DRQN_STASH 192       // floats stashed per source step: i, f, g, o, c, h
template <class T> struct MzDrqnSix {  // torch's LSTMCell / Linear layouts, f32
  T *w_ih, *w_hh, *b_ih, *b_hh, *fc_w, *fc_b;
};
using MzDrqnNet = MzDrqnSix<const float>;  // a net's parameters
using MzDrqnGrads = MzDrqnSix<float>;      // its gradient segments
struct MzDrqnAct {
  MzDrqnNet p;
  const float* obs6; int B, L;               // L == 0: evaluation (no record, every state advances)
  float eps; int explore;                    // explore: actions the uniform draw covers
  uint64_t seed, counter;
  const int32_t* t;
  const float *h, *c; float *h_out, *c_out;  // [32][B]; out may alias in
  float* rec_x; int32_t* rec_a;              // [B][L + 1][6], [B][L]
  int32_t* act_out; float* q_out;            // [B]; [B][4] or null
};
struct MzDrqnStore {
  const float* obs6; const uint8_t* term; int B, L;
  const int32_t* fin_id; const int32_t* fin_len; const int32_t* fin_count;
  float* rec_x; const int32_t* rec_a; const double* rec_r;
  int64_t cap; uint32_t* mem; int32_t* mem_len; int32_t* mem_term;  // [cap][L + 1][8], [cap], [cap]
  int64_t* ring;                             // head, count
};
struct MzDrqnSample {
  uint64_t seed, counter; int E, L; int64_t cap;
  const int64_t* ring; const int32_t* mem_len;
  int32_t* d_slot; int32_t* d_len; int64_t* d_off; int64_t* d_tot;  // [E] x 3; rows, steps
};
// What the whole-episode and the window update share: the net, the replay memory and the row
// buffers (E (L + 1) rows for whole episodes, E (min(T, L) + 2) for windows).
struct MzDrqnUnroll {
  MzDrqnNet p;
  int target, E, L; int64_t cap; float gamma;
  const uint32_t* mem; const int32_t* mem_term;
  float* qmax;                               // [rows] max_a Q'_t (target: out; source: in)
  float* stash; float* qa; float* y; float* d; double* ep_loss;  // source: out; backward: in
  float* gpart;                              // backward: [E][MZ_DRQN_PARAMS]
};
struct MzDrqnSeq {
  MzDrqnUnroll u;
  const int32_t* d_slot; const int32_t* d_len; const int64_t* d_off; const int64_t* d_tot;
};

// Replay windows of T steps with stored state and K burn-in steps. A state snapshot is 64 f32
// (h[32], c[32]); an episode's snapshot j is the state before it acted at step j T (entry 0 is
// never written: zero by definition). The window directory wdir is int32 [5][E]:
#define MZ_DRQN_SNAP 64
#define MZ_DRQN_WDIR_SLOT 0     // ring slot
#define MZ_DRQN_WDIR_LEN 1      // the episode's length n
#define MZ_DRQN_WDIR_B 2        // first unrolled step b = max(0, j T - K)
#define MZ_DRQN_WDIR_K 3        // burn-in steps k = j T - b
#define MZ_DRQN_WDIR_M 4        // training steps m = min(T, n - j T)
#define MZ_DRQN_WIN_PAD 2       // a window's rows: the entry-state row, m step rows, the guard row
struct MzDrqnSnap {
  int B, L, T;
  const int32_t* t; const float *h, *c;      // [B]; [32][B]
  float* snap_rec;                           // [B][ceil(L / T)][64]
};
struct MzDrqnSnapStore {
  int B, L, T;
  const int32_t* fin_id; const int32_t* fin_len; const int32_t* fin_count;
  const float* snap_rec; int64_t cap; float* mem_state;  // [cap][ceil(L / T)][64]
  const int64_t* ring;
};
struct MzDrqnWinSample {
  MzDrqnSample s;                            // s.d_slot / s.d_len: wdir's first two rows
  int T, K;
  int32_t* wdir;
};
struct MzDrqnWin {
  MzDrqnUnroll u;
  int T, K;
  const float* mem_state;                    // null: every window starts from zero state
  const int32_t* wdir; const int64_t* w_off; const int64_t* w_tot;  // rows, training steps
};
hipError_t mz_launch_drqn_snapshot(const MzDrqnSnap& q, hipStream_t s);

// Prioritized replay windows. Window (slot, j) carries a mass: u32 fixed point with
// MZ_DRQN_PRIO_FRAC fractional bits, 0 = no such window. mem_prio [cap][ceil(L / T)], mem_psum
// [cap] = the slot's sum of masses (u64), prio_max [1] = the largest mass an update has written.
// Every sum over masses is an exact 64-bit integer, so no result depends on a reduction's order.
#define MZ_DRQN_PRIO_FRAC 20
#define MZ_DRQN_PRIO_CEIL (1u << 30)  // the largest mass
struct MzDrqnPrioStore {
  int B, L, T;
  const int32_t* fin_id; const int32_t* fin_len; const int32_t* fin_count;
  int64_t cap; uint32_t* mem_prio; uint64_t* mem_psum; const uint32_t* prio_max;
  const int64_t* ring;
};
struct MzDrqnPrioSample {
  uint64_t seed, counter; int E, L, T, K; int64_t cap;
  const int32_t* mem_len; const uint32_t* mem_prio; const uint64_t* mem_psum;
  int32_t* wdir; int64_t* w_off; int64_t* w_tot;  // as MzDrqnWinSample writes them
  float* isw; double beta;                        // [E] importance weights
};
struct MzDrqnPrioUpdate {
  int E, L, T; int64_t cap;
  const int32_t* wdir; const int64_t* w_off; const int64_t* w_tot;
  const float* qa; const float* y; float* d; double* ep_loss;  // the source forward's rows
  const float* isw; double alpha, eta, eps;
  uint32_t* mem_prio; uint64_t* mem_psum; uint32_t* prio_max;
};

// Populations: P independent learners over B = P b instances, learner p owning the block
// [p b, (p + 1) b). Parameters, gradients and moments are flat [P][MZ_DRQN_PARAMS] f32, a row in
// state_dict order. Every stage has one kernel and one launcher, which take the structs below: each
// holds learner 0's single-learner view, and the kernel moves it to learner p's rows. A single
// learner is P = 1, b = B with the per-learner arrays null: where one is null the kernel keeps the
// by-value field of the embedded struct. due: [P], 0 = the learner sits the update out (null: all
// due).
template <class T> inline MzDrqnSix<T> mz_drqn_flat_net(T* f) {  // the six tensors of one flat row
  return MzDrqnSix<T>{f, f + 768, f + 768 + 4096, f + 768 + 4096 + 128, f + 768 + 4096 + 256,
                      f + 768 + 4096 + 256 + 128};
}
struct MzDrqnPopAct {
  MzDrqnAct a;                               // a.B = P b (the pitch of h / c)
  int P, b;
  const float* eps; const uint64_t* seed;    // [P]; null: a.eps, a.seed
};
struct MzDrqnPopStore {
  MzDrqnStore s;                             // s.B = P b; mem [P][cap][L + 1][8], ring [P][2]
  int P, b;
};
struct MzDrqnPopSample {
  MzDrqnSample s;                            // directory [P][E], d_tot [P][2]
  int P;
  const uint64_t* seed; const uint64_t* counter;  // [P]; null: s.seed, s.counter
  const int32_t* due;                        // [P]
};
struct MzDrqnPopSeq {
  MzDrqnSeq q;                               // row buffers [P][E (L + 1)], gpart [P][E][5252]
  int P;
  const float* gamma; const int32_t* due;    // [P]; gamma null: q.u.gamma
};
struct MzDrqnReduce {
  int P, E, ld;                              // ld: int32 words between two learners' d_len rows
  const float* gpart; const double* ep_loss; const int32_t* d_len; const int64_t* d_tot;
  MzDrqnGrads g;                             // learner 0's gradient segments; learner p's are
  float* loss; const int32_t* due;           // MZ_DRQN_PARAMS floats further on each; [P], [P]
};
// Replay windows in a population: T is shared (it fixes the layouts), the burn-in K_p and whether
// the state memory is read are per learner. The window directory is one [5][E] block per learner.
struct MzDrqnPopSnapStore {
  MzDrqnSnapStore s;                         // s.B = P b; mem_state [P][cap][ceil(L / T)][64], ring [P][2]
  int P, b;
};
struct MzDrqnPopWinSample {
  MzDrqnWinSample w;                         // wdir [P][5][E], d_off [P][E], d_tot [P][2]; w.K = K_max
  int P;
  const uint64_t* seed; const uint64_t* counter;  // [P]; null: w.s.seed, w.s.counter
  const int32_t* burn_in; const int32_t* due;     // [P]; burn_in null: w.K, which the host checked
};
struct MzDrqnPopWin {
  MzDrqnWin q;                               // row buffers [P][E (min(T, L) + 2)]; q.K = K_max
  int P;
  const float* gamma; const int32_t* burn_in;  // [P]; null: q.u.gamma, q.K
  const int32_t* stored; const int32_t* due;   // [P]; stored null: q.mem_state as given
};
// Prioritized windows in the per-learner row form: mem_prio [P][cap][ceil(L / T)], mem_psum
// [P][cap], prio_max [P], isw [P][E]; the directory and the row buffers as MzDrqnPopWin's.
struct MzDrqnPopPrioStore {
  MzDrqnPrioStore s;                         // s.B = P b
  int P, b;
};
struct MzDrqnPopPrioSample {
  MzDrqnPrioSample s;                        // s.K = K_max
  int P;
  const uint64_t* seed; const uint64_t* counter;  // [P]; null: s.seed, s.counter
  const int32_t* burn_in; const int32_t* due;     // [P]; burn_in null: s.K
  const double* beta;                             // [P]; null: s.beta
};
struct MzDrqnPopPrioUpdate {
  MzDrqnPrioUpdate u;
  int P;
  const int32_t* due;                        // [P]
  const double* alpha; const double* eta; const double* eps;  // [P]; null: u.alpha, u.eta, u.eps
};
// Double-Q targets and n-step returns: the forwards' second form and the kernel that forms y, d and
// ep_loss from their rows. q4 [P][rows][4]: the target net's four Q' of a row; sel [P][rows]: the
// first argmax of the source net's own Q. Both cover a span's rows row .. row + m. The embedded
// forward structs are filled as for the old forwards, with qmax, y, d and ep_loss null there.
struct MzDrqnQRows {
  float* q4; int32_t* sel;                   // target form: q4 out; source form: sel out
};
struct MzDrqnPopSeqQ {
  MzDrqnPopSeq q; MzDrqnQRows x;
};
struct MzDrqnPopWinQ {
  MzDrqnPopWin q; MzDrqnQRows x;
};
struct MzDrqnReturns {
  const int32_t* n_step; int n_max;          // [P]; a value outside 1 .. n_max counts as the nearer bound
  const int32_t* dbl;                        // [P], 0 = bootstrap from max q4 (null: all read sel)
  const float* q4; const int32_t* sel;       // sel null: every learner bootstraps from max q4
};
struct MzDrqnPopSeqRet {
  MzDrqnPopSeq q; MzDrqnReturns r;           // q.q.u: mem, mem_term, qa (in), y, d, ep_loss (out)
};
struct MzDrqnPopWinRet {
  MzDrqnPopWin q; MzDrqnReturns r;
};
// target != 0 in the embedded struct: the target form
hipError_t mz_launch_drqn_seq_forward_q(const MzDrqnPopSeqQ& q, hipStream_t s);
hipError_t mz_launch_drqn_window_forward_q(const MzDrqnPopWinQ& q, hipStream_t s);
hipError_t mz_launch_drqn_seq_returns(const MzDrqnPopSeqRet& q, hipStream_t s);
hipError_t mz_launch_drqn_window_returns(const MzDrqnPopWinRet& q, hipStream_t s);
hipError_t mz_launch_drqn_prio_store(const MzDrqnPopPrioStore& q, int blocks, hipStream_t s);
hipError_t mz_launch_drqn_prio_sample(const MzDrqnPopPrioSample& q, hipStream_t s);
hipError_t mz_launch_drqn_prio_update(const MzDrqnPopPrioUpdate& q, hipStream_t s);
// blocks: the store's workgroups per learner
hipError_t mz_launch_drqn_act(const MzDrqnPopAct& q, hipStream_t s);
hipError_t mz_launch_drqn_store(const MzDrqnPopStore& q, int blocks, hipStream_t s);
hipError_t mz_launch_drqn_sample(const MzDrqnPopSample& q, hipStream_t s);
hipError_t mz_launch_drqn_seq_forward(const MzDrqnPopSeq& q, hipStream_t s);
hipError_t mz_launch_drqn_seq_backward(const MzDrqnPopSeq& q, hipStream_t s);
hipError_t mz_launch_drqn_reduce(const MzDrqnReduce& q, hipStream_t s);
hipError_t mz_launch_drqn_pop_sync(const float* src, float* dst, const int32_t* mask, int P,
                                   hipStream_t s);
hipError_t mz_launch_drqn_snap_store(const MzDrqnPopSnapStore& q, int blocks, hipStream_t s);
hipError_t mz_launch_drqn_window_sample(const MzDrqnPopWinSample& q, hipStream_t s);
hipError_t mz_launch_drqn_window_forward(const MzDrqnPopWin& q, hipStream_t s);
hipError_t mz_launch_drqn_window_backward(const MzDrqnPopWin& q, hipStream_t s);
// mz_optim.hip: k_adamw's element arithmetic over [P][n] rows with per-learner lr / step / due
hipError_t mz_launch_adamw_pop(float* p, float* m, float* v, float* g, int P, int64_t n,
                               const float* lr, float* step, const int32_t* due, double b1,
                               double b2, double eps, double wd, float clamp, float gscale,
                               int write_grad, hipStream_t s);

// ---- f32-accurate acting forward on the bf16 MFMA (mz_qact.hip) ------------------------------
struct MzQAct {
  const uint32_t* bits; const float* obs6;   // [B][22], [B][6] (instance rows)
  const int32_t* rows; const int32_t* count; int n;  // rows[i] (i < min(n, *count)) or row i
  const float* conv_w; const float* conv_b;  // [32][27], [32]
  const uint16_t* w1h; const uint16_t* w1l; const float* b1;  // prepared [1024][1600] bf16, [1024]
  const uint16_t* w2h; const uint16_t* w2l; const float* b2;  // prepared [512][1024] bf16, [512]
  const float* w3; const float* b3;          // [4][512], [4]
  uint32_t drop_thresh; float drop_scale; uint32_t key;
  float* h1;                                 // workspace [n][1024] f32
  int64_t* greedy; float* q_out;             // greedy[inst] = argmax; q_out [n][4] (nullable)
};
int mz_qact_row_tiles(int n);
int64_t mz_qact_ws_floats(int n);
hipError_t mz_launch_qact(const MzQAct& q, int relu, hipStream_t s);
hipError_t mz_launch_qact_prepare(const float* w1, const float* w2, uint16_t* w1h, uint16_t* w1l,
                                  uint16_t* w2h, uint16_t* w2l, hipStream_t s);

// ---- vectorised tabular learners: Q and double Q, dense or hashed tables (mz_qtab.hip) --------
struct MzQtabAct {
  const float* obs6; int n, P;               // plain observations [n][6], pitch of the index
  const int32_t* table_of; int T;            // instance -> table (null: i), tables
  const uint8_t* active;                     // [n] 0 = the instance idles (null: all act)
  const double* q; int64_t rows;             // dense: [T][rows][4] f64; hashed: null, rows stays
                                             // 5 P^4, the key range
  const long long* steps_done;               // [T]
  const double* eps_init; const double* eps_final; const double* eps_decay;  // [T]
  uint64_t seed, counter;
  int32_t* actions; int64_t* sidx;           // [n] action taken, row index acted from
};
struct MzQtabUpd {
  const float* obs6; int n, P;               // the step's next observations
  const int32_t* table_of; int T;
  double* q; int64_t rows;
  const int64_t* sidx; const int32_t* actions;
  const double* reward64; const uint8_t* terminated; const uint8_t* truncated;
  double* gamma; const double* lr; const double* eta;  // [T]
  double* cum;                               // [n] episode's cumulative reward
  long long* episodes; long long* wins;      // [T]
  double* td;                                // [n] lr * td between the two shared-table passes
  int episode_end;                           // 0: QAgent.update alone (no gamma drift, no counters)
};
// hashed tables of the same learners
struct MzQhash {
  int32_t* keys;                             // [T][C] dense state index, -1 = empty
  double* vals;                              // [T][C][4] f64, zero until written
  int32_t* load; long long* overflow;        // [T] occupied slots, dropped updates
  uint32_t C; int shift;                     // capacity (a power of two), 32 - log2 C
};
// double Q-learning. A state's A row and B row sit side by side, [2][4] f64 = 64 B: MzQtabAct::q / MzQtabUpd::q are
// [T][rows][2][4] and MzQhash::vals is [T][C][2][4] (64-B aligned).
struct MzDqtabUpd {
  MzQtabUpd u;                               // u.td: lr * td between the two shared-table passes
  const long long* steps_done;               // [T] as the update finds it (after the act's advance)
  const double* eps_init; const double* eps_final; const double* eps_decay;  // [T]
  uint64_t seed, ucounter;                   // ucounter: the agent's count of update calls
  const uint8_t* coin;                       // [n] 0 = A, 1 = B (null: draw)
  const int32_t* next_action;                // [n] in 0..3 (null: the inner eps-greedy choice)
  uint8_t* took;                             // [n] 1 where a td was computed
  uint8_t* which;                            // [n] the table updated, between the shared passes
};
// One launcher per stage. width: 1 = Q-learning, 2 = double Q. h: the hashed tables (null: dense,
// a.q / d.u.q). act: k_qtab_act (double Q: on the A row), then the advance. update: independent
// tables one launch, shared tables two (td, apply); Q-learning reads d.u alone; double Q then
// advances steps_done by took, for the inner get_actions.
hipError_t mz_launch_qtab_act(const MzQtabAct& a, int width, const MzQhash* h,
                              long long* steps_done, hipStream_t s);
hipError_t mz_launch_qtab_update(const MzDqtabUpd& d, int width, const MzQhash* h,
                                 long long* steps_done, hipStream_t s);
hipError_t mz_launch_qtab_advance(const int32_t* table_of, const uint8_t* active, int n, int T,
                                  long long* steps_done, hipStream_t s);
hipError_t mz_launch_qtab_rehash(const MzQhash& from, const MzQhash& to, int T, int width,
                                 hipStream_t s);
hipError_t mz_launch_qtab_lookup(const MzQhash& h, int T, int width, const int32_t* tables,
                                 const int64_t* keys, int m, double* rows_out, int32_t* slots_out,
                                 hipStream_t s);
