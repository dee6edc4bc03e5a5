/* mazerl.h — C ABI of libmazerl.so, the MI355X-native batched maze environment.
 *
 * The reference (Fabri000/Maze-Solving-Agent-Gymnasium) has no FFI: its boundary is the Python
 * gym.Env class API. This header is the drop-in boundary underneath that API:
 * the Python classes in maze-solving-agent-gymnasium_amd/mazerl/ bind these entry points with
 * ctypes (INTEGRATION.md shows the binding). Each entry point names the reference interface it
 * replaces (file:line in the reference).
 *
 * Conventions
 *   - Every call returns an int status: MZ_OK (0) or a negative MZ_E* code; mz_last_error()
 *     returns the thread-local message of the last failure.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream). Calls are async on it
 *     unless documented as synchronous.
 *   - Pointers named *_dev are device (HBM) pointers owned by the caller (e.g. torch tensors);
 *     pointers named *_host are host pointers. The handle owns all per-instance env state.
 *   - One handle per stream/thread; handles are not internally locked. Instances (envs) of a
 *     handle are fully independent (no global mutable state, per-instance algorithm id).
 *   - Grids are uint8, row-major, 0 = wall, 1 = floor, 2 = goal (lib/maze_generation.py:16).
 *     Shapes must be square and odd (the reference raises IndexError for even N),
 *     5 <= N <= MZ_MAX_DIM. Window (enrich) mode needs N >= 15 for euclidean mazes (Q7).
 */
#ifndef MAZERL_H
#define MAZERL_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MZ_OK 0
#define MZ_EINVAL (-1)       /* bad argument */
#define MZ_EINVAL_SHAPE (-2) /* grid shape the reference cannot represent (even N, N<15 window) */
#define MZ_EHIP (-3)         /* HIP runtime error */
#define MZ_ENOMEM (-4)
#define MZ_EALIGN (-5)       /* output pointer misaligned (window f32 needs 16 B) */

#define MZ_MAX_DIM 127
#define MZ_BANK_MAX_DIMS 64  /* maze sizes one bank can hold (mz_bank_create_dims) */
#define MZ_MAX_CANDIDATES 64 /* candidates of a best-of-C selection (mz_bank_create_ex, mz_generate_best) */
#define MZ_WINDOW 15
#define MZ_WINDOW_BITS 675   /* 3 x 15 x 15 */
#define MZ_WINDOW_WORDS 22   /* uint32 words per instance in window_bits (bits 675..703 zero) */

/* algorithm ids (BaseMazeEnv.ALGORITHM strings, base_maze_env.py:17; maze_generation.py:24-30) */
#define MZ_ALGO_RPRIM 0
#define MZ_ALGO_DFS 1
#define MZ_ALGO_PRIMKILL 2

typedef struct mz_handle mz_handle;

typedef struct {
  int32_t num_envs;  /* B: independent env instances on this GPU */
  int32_t max_dim;   /* storage pitch: every instance's N <= max_dim */
  int32_t toroidal;  /* 0 euclidean (SimpleMazeEnv family), 1 toroidal (ToroidalMazeEnv family) */
  int32_t enrich;    /* 1 = *Enrich* observation (3x15x15 window), 0 = plain obs */
  int32_t device;    /* HIP device ordinal */
  int32_t reserved[7];
} mz_config;

/* Per-step outputs; every pointer is a caller-owned device buffer and may be NULL (= not
 * written). Reward dtype note: the reference returns Python floats/ints; reward64 carries the
 * exact value, reward is its float32 rounding (what torch.tensor(batch.reward) holds). */
typedef struct {
  float* reward;          /* [B] */
  double* reward64;       /* [B] */
  uint8_t* terminated;    /* [B] */
  uint8_t* truncated;     /* [B] */
  int32_t* pos;           /* [B][2] agent (row, col)           obs["agent"] (plain) */
  int32_t* best_dir;      /* [B][2] agent - best_next_cell     obs["best dir"] */
  float* obs6;            /* [B][6] learner state vector concat(agent, target, best dir) as f32,
                             enrich: agent/maze_shape, target/maze_shape (off_policy_trainer.py:156) */
  uint32_t* window_bits;  /* [B][22] 675-bit 3x15x15 window, channel-major, LSB-first */
  float* window;          /* [B][3][15][15] f32 obs["window"] (get_mask_tensor), 16 B aligned */
  int32_t* done_idx;      /* [B] indices of instances whose step ended terminated|truncated */
  int32_t* done_count;    /* [1] number of valid done_idx entries (caller zeroes it first) */
} mz_step_out;

typedef struct { /* host-side snapshot of one instance (mz_query) */
  int32_t n, start_r, start_c, goal_r, goal_c, max_steps;
  int32_t r, c, steps, invalid_streak, nmoves, last_action, done;
} mz_env_info;

const char* mz_last_error(void);
int mz_device_count(int* n);

/* Create / destroy a batch of B env instances on one GPU. */
int mz_create(const mz_config* cfg, mz_handle** out);
int mz_destroy(mz_handle* h);

/* Import mazes bit-exactly (e.g. reference-generated fixtures) into instances env_ids_host[i]
 * (NULL = 0..n-1). grids_host is [n][dim][dim]; start_goal_host is [n][4] (sr, sc, gr, gc).
 * Builds the per-maze distance field / move tables, max_steps, and resets the instances.
 * Replaces: env construction with a given maze (SimpleMazeEnv.__init__, simple_maze_env.py:19-36)
 * and set_max_steps (:52-58). Synchronous. */
int mz_load_mazes(mz_handle* h, const uint8_t* grids_host, int32_t dim,
                  const int32_t* start_goal_host, const int32_t* env_ids_host, int32_t n,
                  void* stream);

/* Generate new mazes on the GPU for the listed instances (env_ids_dev NULL = all B) with the
 * per-instance algorithm ids (algo_dev [n] or NULL = algo_all) and Philox seeds
 * seed + env_id; then builds tables and resets them. Replaces gen_maze / gen_maze_no_border
 * (maze_generation.py:6-56) + update_new_maze (simple_maze_env.py:118-127) with candidates=1
 * (the best-of-6 difficulty selection, base_maze_env.py:78-97, is mz_generate_best). */
int mz_generate(mz_handle* h, const int32_t* env_ids_dev, int32_t n, const uint8_t* algo_dev,
                int32_t algo_all, int32_t dim, uint64_t seed, void* stream);

/* Best-of-C generation: the reference's new-maze selection (BaseMazeEnv.generate_maze,
 * base_maze_env.py:78-97; ToroidalMazeEnv.generate_maze, toroidal_maze_env.py:40-54: six
 * gen_maze / gen_maze_no_border candidates, the one with the smallest McClendon difficulty —
 * maze_complexity_evaluation.py:319-329, a toroidal maze scored as its bordered maze — kept, the
 * first on ties) for the listed instances, on the GPU: `candidates` Philox mazes per instance
 * (candidate c of instance e: seed + e * candidates + c, the mazes mz_generate of
 * n * candidates instances from `seed` builds for instances e * candidates + c), scored by the
 * difficulty kernel, the first minimum copied into the instance (which is then reset like after
 * mz_generate). Euclidean handles score every candidate first with the order-free screen
 * (mz_screen_batch) and decide a group from it when its minimum is separated from every other
 * candidate by more than the screen's rigorous error bounds (+ 2^-40); the other groups are
 * rebuilt and scored by the order-exact kernel (mz_difficulty_batch), and a candidate that kernel
 * declines is scored by the host restatement (mz_difficulty) inside the stream
 * (hipLaunchHostFunc), so every candidate of a group is compared. candidates == 1 is
 * mz_generate_ex(MZ_RNG_PHILOX). Selection statistics:
 * mz_select_stats. Replaces update_new_maze (simple_maze_env.py:118-127) / the env constructors'
 * first maze (simple_maze_env.py:19-36). */
int mz_generate_best(mz_handle* h, const int32_t* env_ids_dev, int32_t n, const uint8_t* algo_dev,
                     int32_t algo_all, int32_t dim, uint64_t seed, int32_t candidates,
                     void* stream);
/* Counters of every best-of-C selection on this handle (bank refills and mz_generate_best) ->
 * out3_dev [3] int32 (device, nullable): groups with a candidate the GPU difficulty kernel leaves
 * to the host (status != 0; the group picks among the others), groups where a candidate listed
 * before the chosen one lies within a relative 2^-40 of its difficulty product (its log could
 * tie the chosen one's: the reference would keep the earlier), groups selected. reset != 0 zeroes
 * them after the copy. */
int mz_select_stats(mz_handle* h, int32_t* out3_dev, int32_t reset, void* stream);
/* The same counters, the first n (<= MZ_SELECT_STATS) of: [0] unresolved groups (a candidate
 * with no score from the GPU kernels or the host — or a group past the exact path's per-run cap
 * of 256, which keeps the screen's pick), [1] near ties (as above), [2] groups selected, [3]
 * groups the screen left to the order-exact kernel, [4] candidates scored by the host
 * restatement. */
#define MZ_SELECT_STATS 5
int mz_select_stats_ex(mz_handle* h, int32_t* out_dev, int32_t n, int32_t reset, void* stream);
/* Test hooks of the best-of-C pipeline (flags, 0 = off): 1 every group to the order-exact
 * kernel, 2 even-numbered candidates treated as declined by it (host-scored), 4 all candidates of
 * a group from one seed (exact ties). */
int mz_set_debug(mz_handle* h, int32_t flags);
/* Per-instance size of a winner's next maze for mz_reset_done / mz_reset_list with regen_won:
 * dims_dev [B] uint8 (device, owned by the caller, read by every later reset launch; NULL = each
 * instance's current size, the default). 0 = the winner keeps its maze and is only reset — the
 * variable-size envs' update_maze when `shape + 4 > max_shape` (simple_variable_maze_env.py:93-112,
 * toroidal_variable_maze_env.py:113-131), which leaves the maze as it is. A value the handle cannot
 * hold (even, < 5, > max_dim) counts as 0. */
int mz_set_regen_dims(mz_handle* h, const uint8_t* dims_dev);

/* rng of mz_generate_ex:
 *   MZ_RNG_PHILOX   Philox4x32 stream seed + env_id (as mz_generate): every random choice of the
 *                   reference is drawn uniformly over the same candidates (distribution parity).
 *   MZ_RNG_CPYTHON  CPython-exact: instance env_id gets the maze the reference builds with
 *                   `random.seed(seed + env_id); gen_maze((dim, dim), algo)` (toroidal:
 *                   gen_maze_no_border), bit for bit — MT19937 draws and CPython 3.10 set
 *                   iteration order emulated on the GPU (maze_generation.py:6-185). */
#define MZ_RNG_PHILOX 0
#define MZ_RNG_CPYTHON 1
int mz_generate_ex(mz_handle* h, const int32_t* env_ids_dev, int32_t n, const uint8_t* algo_dev,
                   int32_t algo_all, int32_t dim, uint64_t seed, int32_t rng, void* stream);

/* One CPython-exact maze for instance `env` from an explicit Python random state:
 * state_host[625] = random.getstate()[1] (624 MT19937 words + index), advanced in place exactly
 * as gen_maze((dim, dim), algo) would advance Python's global random (the caller writes it back
 * with random.setstate). Used by the single-env drop-in classes so that random.seed(s) before
 * construction gives the reference's maze (base_maze_env.py:78-97 draws six candidates from the
 * global stream). Synchronous. */
int mz_generate_state(mz_handle* h, int32_t env, int32_t dim, int32_t algo, uint32_t* state_host,
                      void* stream);

/* Reset every instance / a device list of instances (e.g. step's done_idx/done_count) and
 * write their reset observations into `out`. Replaces BaseMazeEnv.reset (base_maze_env.py:136-161).
 * A non-NULL count_dev is consumed: the kernel sets it to 0 once every workgroup has read it,
 * so the next mz_step_act may pass MZ_STEP_COUNT_ZEROED.
 * With regen_won != 0, listed instances whose last step terminated get a freshly generated maze
 * first (the trainer's win -> update_maze protocol, off_policy_trainer.py:190-202), using their
 * stored algorithm id and seed + env_id + (epoch << 32). */
int mz_reset_all(mz_handle* h, const mz_step_out* out, void* stream);
int mz_reset_list(mz_handle* h, const int32_t* idx_dev, const int32_t* count_dev,
                  int32_t max_count, int32_t regen_won, uint64_t seed, uint32_t epoch,
                  const mz_step_out* out, void* stream);

/* Auto-reset: reset every instance whose last step ended terminated|truncated (a per-instance
 * flag kept by the step; no device list needed) and write its reset observation into `out`.
 * With regen_won != 0 the instances that won get a new maze first (as mz_reset_list). */
int mz_reset_done(mz_handle* h, int32_t regen_won, uint64_t seed, uint32_t epoch,
                  const mz_step_out* out, void* stream);

/* One env step for all B instances. actions_dev: [B] int32 in 0..3 (BaseMazeEnv.ACTIONS);
 * a negative action means "observe only": no transition, outputs = observation of the current
 * state with reward 0 and terminated = truncated = 0 (used to step a subset of instances).
 * Replaces BaseMazeEnv.step (base_maze_env.py:163-210) with the move rule of
 * maze_view.move_agent (maze_view.py:167-197) and _get_obs/_find_best_next_cell (:116-122,
 * :224-262) / the Enrich window (maze_handler.py:4-99). */
int mz_step(mz_handle* h, const int32_t* actions_dev, const mz_step_out* out, void* stream);

/* flags of mz_step_ex / mz_step_act:
 *   MZ_STEP_COUNT_ZEROED  out->done_count is already 0 (skip the memset).
 *   MZ_STEP_AUTORESET     an instance whose previous step ended terminated|truncated is reset
 *                         by this launch instead of stepping (BaseMazeEnv.reset,
 *                         base_maze_env.py:136-161, same maze: the reference trainer's
 *                         env.reset() at the top of the next episode,
 *                         off_policy_trainer.py:153). Its action is ignored (actions_out = -1),
 *                         reward 0, terminated = truncated = 0, outputs = the reset
 *                         observation. One launch per vector step instead of step +
 *                         mz_reset_done. */
#define MZ_STEP_COUNT_ZEROED 1
#define MZ_STEP_AUTORESET 2
/* mz_step with flags. */
int mz_step_ex(mz_handle* h, const int32_t* actions_dev, const mz_step_out* out, int32_t flags,
               void* stream);

/* Fused act + step (one launch): each instance takes the epsilon-greedy action of mz_act
 * (below) and steps; actions_out_dev [B] (nullable) receives the actions taken. */
int mz_step_act(mz_handle* h, const float* eps_dev, float eps_all, const int64_t* greedy_dev,
                uint64_t seed, uint64_t counter, int32_t* actions_out_dev, const mz_step_out* out,
                int32_t flags, void* stream);

/* get_mask_direction(probs) for all instances: out4_dev [B][4] f32
 * (simple_maze_env.py:41-50, toroidal_maze_env.py:57-69). */
int mz_direction_mask(mz_handle* h, int32_t probs, float* out4_dev, void* stream);

/* Fused epsilon-greedy act (dqn_agent.py:104-116): for instance i, with u ~ U[0,1)
 * (Philox(seed, i, counter)), if u < eps[i] (eps_dev NULL = eps_all) sample from the
 * normalised get_mask_direction(probs=True) distribution, else take greedy_dev[i]
 * (NULL = always explore). Writes actions_dev [B] int32. */
int mz_act(mz_handle* h, const float* eps_dev, float eps_all, const int64_t* greedy_dev,
           uint64_t seed, uint64_t counter, int32_t* actions_dev, void* stream);

/* Expand n packed windows (window_bits layout) to f32 [n][3][15][15]. */
int mz_expand_window(const uint32_t* bits_dev, float* out_dev, int32_t n, void* stream);

/* Maze bank: regeneration on win (update_maze, simple_maze_env.py:81-94, called from
 * off_policy_trainer.py:190-202) copies a maze generated ahead of time instead of building one
 * inside mz_reset_done (one build is a ~1 ms serial chain: carve loop + two level-synchronous
 * BFS; a copy is a few microseconds). Two banks of `slots` mazes per algorithm in algo_mask
 * (bit a = algorithm id a), all of size `dim`; the caller consumes one (mz_bank_use) while it
 * refills the other (mz_bank_fill, e.g. on a side stream ordered after the consuming launches).
 * Mazes: Philox seed ^ ((3*bank + algo + 1) << 56) + slot + (fill epoch << 32). An exhausted
 * bank, or an instance whose algorithm / size the bank lacks, falls back to building in place. */
int mz_bank_create(mz_handle* h, int32_t slots, int32_t dim, uint32_t algo_mask);
/* The same for a list of ndims (<= MZ_BANK_MAX_DIMS) distinct maze sizes: `slots` mazes per
 * (algorithm, size) — the variable-size envs (config 5: toroidal 17..79, instance i of size
 * dims[i mod n]); a win copies a maze of the instance's own size. Size index di keys its slots'
 * Philox seeds with di << 48 (di = 0: mz_bank_create's). */
int mz_bank_create_dims(mz_handle* h, int32_t slots, const int32_t* dims, int32_t ndims,
                        uint32_t algo_mask);
/* mz_bank_create_dims whose slots are best-of-`candidates` mazes (1..MZ_MAX_CANDIDATES): every
 * refilled slot is the easiest of `candidates` mazes by McClendon difficulty, the first on ties —
 * the reference's generate_maze selection for the new maze of a win (base_maze_env.py:78-97,
 * toroidal_maze_env.py:40-54, via update_maze at off_policy_trainer.py:202 / ppo_trainer.py:96).
 * Candidate c of slot j of a fill: Philox key + j * candidates + c + (epoch << 32) with the
 * block's key as mz_bank_fill's (candidates = 1: mz_bank_create_dims exactly). Needs the
 * difficulty kernel's LDS plan (max_dim <= 91 euclidean, <= 89 toroidal) when candidates > 1;
 * the K * candidates candidate mazes live in scratch owned by the handle. */
int mz_bank_create_ex(mz_handle* h, int32_t slots, const int32_t* dims, int32_t ndims,
                      uint32_t algo_mask, int32_t candidates);
/* Rebuild the slots of `bank` consumed since its last fill (every slot on the first fill). */
int mz_bank_fill(mz_handle* h, int32_t bank, uint64_t seed, void* stream);
/* Inspect one bank slot (synchronous; tests): the grid (0 wall, 1 floor, 2 goal) into
 * grid_host [N][N] (N = the slot's size, <= max_dim) and (start r, start c, goal r, goal c). */
int mz_bank_slot_grid(mz_handle* h, int32_t bank, int32_t algo, int32_t size_index, int32_t slot,
                      uint8_t* grid_host, int32_t* info4_host);
/* Bank consumed by later mz_reset_done(regen_won) launches; -1 = none (build in place). */
int mz_bank_use(mz_handle* h, int32_t bank);
/* Consumed-slot counters of `bank` per algorithm id and size index -> out3_dev [3][ndims] int32
 * (device; [3] for a single-size bank). */
int mz_bank_consumed(mz_handle* h, int32_t bank, int32_t* out3_dev, void* stream);

/* Checkpoint / resume of a handle's env state (the reference has none; its envs keep
 * their mazes in Python lists, simple_maze_env.py:34,91). One device buffer holds a 256-B header
 * (magic "MZST", version, B, P, toroidal, enrich, the bank geometry, the active bank and its fill
 * epochs) and every per-instance array of the handle — cell words (maze, BFS table, visit counts
 * and tags), open / visited plane strips, meta, position / step / current-cell words, algorithm
 * ids, last-terminated flags — plus, when the handle has a maze bank, both banks with their
 * consumed-slot counters. mz_state_bytes: the buffer size; mz_state_save: device-to-device copies
 * on `stream`; mz_state_load: validates the header against the handle (same num_envs, max_dim,
 * toroidal, enrich; the same bank geometry, created with mz_bank_create*; MZ_EINVAL otherwise),
 * then copies back and re-activates the saved bank. Stepping a loaded handle continues
 * bit-exactly where the saved one stood. */
#define MZ_STATE_HEADER_BYTES 256
int mz_state_bytes(mz_handle* h, uint64_t* bytes_out);
int mz_state_save(mz_handle* h, void* dst_dev, uint64_t bytes, void* stream);
int mz_state_load(mz_handle* h, const void* src_dev, uint64_t bytes, void* stream);

/* Fused conv stem of the DQN/DDQN Q-network for acting (dqn_agent.py:19-57 forward,
 * ddqn_agent.py:18-52): from n packed windows (window_bits layout) and obs6 [n][6] f32, writes
 * feat_dev [n][ld] bf16 = [MaxPool2(Dropout(LeakyReLU(Conv3x3(window) + b))) (1,568 values,
 * position-major: element q*32 + c = channel c at pooled position q; torch's flatten order is
 * c*49 + q, so fc1's weight columns are permuted once by the caller) | obs6 (6) | zeros], the
 * input row of the first Linear layer.
 * conv_w_dev f32 [32][3][3][3], conv_b_dev f32 [32]; drop_p = 0 (DQN) or the Dropout p (DDQN in
 * train mode), masks drawn from (seed, counter); ld in 1576..1600, multiple of 8. */
int mz_q_front(const uint32_t* bits_dev, const float* obs6_dev, int32_t n, const float* conv_w_dev,
               const float* conv_b_dev, float drop_p, uint64_t seed, uint64_t counter,
               uint16_t* feat_dev, int32_t ld, void* stream);

/* mz_q_front over a row list: output row i is instance rows_dev[i] (i < n) of bits_dev / obs6_dev;
 * with count_dev (nullable) the rows i < min(n, *count_dev), the length read on the device (the
 * stem can run before the caller knows the list's length). With the list of mz_greedy_rows the
 * acting forward runs over the rows that act greedily only (dqn_agent.py:104-116 evaluates
 * source_net(state) only when `sample >= eps`). */
int mz_q_front_rows(const uint32_t* bits_dev, const float* obs6_dev, const int32_t* rows_dev,
                    const int32_t* count_dev, int32_t n, const float* conv_w_dev,
                    const float* conv_b_dev, float drop_p, uint64_t seed, uint64_t counter,
                    uint16_t* feat_dev, int32_t ld, void* stream);

/* Greedy-row list of the next fused act (mz_act / mz_step_act with the same eps, seed, counter;
 * dqn_agent.py:104-116 draws `sample = random.random()` first and acts greedily iff
 * sample >= eps): rows_dev[0 .. count) = the instances i < n that will take greedy_dev[i], in
 * increasing order; count_dev [1] int32 (device) and, if count_host is not NULL, the same count
 * into mapped host memory (mz_host_alloc) for the caller's GEMM sizes. scratch_dev: int32
 * [ceil(n / 1024)]. Two launches, no atomics: the list is deterministic. */
int mz_greedy_rows(const float* eps_dev, float eps_all, uint64_t seed, uint64_t counter, int32_t n,
                   int32_t* scratch_dev, int32_t* rows_dev, int32_t* count_dev,
                   int32_t* count_host, void* stream);

/* The same conv stem in f32 for the LEARNER update (optimize_model, dqn_agent.py:121-157,
 * ddqn_agent.py:113-152; forward dqn_agent.py:47-57), forward and backward, from packed windows:
 * feat_dev [n][ld] f32 = [MaxPool2(Dropout(LeakyReLU(Conv3x3(window) + b))) in torch's flatten
 * order (c*49 + q) | obs6], ld >= 1574, i.e. the f32 input of fc.0. drop_p = 0 (DQN) or the
 * Dropout p (DDQN); the mask key is read from rng_dev (a device u64 the caller advances between
 * calls, so a captured HIP graph draws fresh masks on every replay) mixed with `salt`.
 * Dropout rule, the same in mz_stem_forward and mz_stem_backward*: thresh = floor(p * 65536 + 0.5)
 * in f32; a position is kept iff its 16-bit draw >= thresh, and kept values (forward) / gradients
 * (backward) are multiplied by scale = (float)(1 / (1 - (double)p)) when thresh > 0 and by 1 when
 * thresh == 0 — so 0 < p < 2^-17, which can drop nothing, is the stem without dropout in both
 * directions (rng_dev is still required for p > 0, but not read), and p >= 1 - 2^-17 drops every
 * position (features +-0, code bytes 0).
 * code_dev [n][1568] u8 (NULL when no backward follows): per feature the pooled argmax (bits
 * 0-1) and its gradient class (bits 2-3: 0 dropped, 1 kept with a > 0, 2 kept with a <= 0). */
int mz_stem_forward(const uint32_t* bits_dev, const float* obs6_dev, int32_t n,
                    const float* conv_w_dev, const float* conv_b_dev, float drop_p,
                    const uint64_t* rng_dev, uint32_t salt, float* feat_dev, int32_t ld,
                    uint8_t* code_dev, void* stream);
/* Conv weight / bias gradients from the gradient of the stem output gfeat_dev [n][ld] f32 (its
 * first 1,568 columns) and the forward's code bytes: dw_dev [32][3][3][3], db_dev [32] f32
 * (overwritten). partial_dev: workspace of mz_stem_workspace_floats(n) floats. */
int mz_stem_backward(const uint32_t* bits_dev, const uint8_t* code_dev, const float* gfeat_dev,
                     int32_t ld, int32_t n, float drop_p, float* partial_dev, float* dw_dev,
                     float* db_dev, void* stream);
/* mz_stem_backward that also advances the device u64 rng_advance_dev by one after the gradient
 * launches (NULL: nothing advanced): a learner whose nets read one dropout counter in every
 * forward of an update moves it on from the backward, with no launch of its own per forward. */
int mz_stem_backward_ex(const uint32_t* bits_dev, const uint8_t* code_dev, const float* gfeat_dev,
                        int32_t ld, int32_t n, float drop_p, float* partial_dev, float* dw_dev,
                        float* db_dev, uint64_t* rng_advance_dev, void* stream);
int mz_stem_workspace_floats(int32_t n);

/* The convolutional autoencoder that pre-trains that stem (lib/models/convolutional_autoencoder.py,
 * train_CAE.py): decoder ConvTranspose2d(32, 3, kernel 2, stride 2, output_padding 1) -> Sigmoid
 * over the stem's features feat_dev [n][ld] f32 (first 1,568 columns, c*49 + 7i + j; ld >= 1568),
 * dec_w_dev [32][3][2][2], dec_b_dev [3]. mz_cae_decode writes Y [n][3][15][15] f32. */
int mz_cae_decode(const float* feat_dev, int32_t ld, int32_t n, const float* dec_w_dev,
                  const float* dec_b_dev, float* out_dev, void* stream);
/* The reconstruction loss alpha * MSE(Y, X) + (1 - alpha) * (1 - SSIM(Y, X)) against the packed
 * windows bits_dev [n][22] (bit ch*225 + r*15 + c of a sample is X[ch][r][c]); SSIM with an 11-tap
 * Gaussian (sigma 1.5) filtered without padding (15x15 -> 5x5), C1 = 0.01^2, C2 = 0.03^2, the mean
 * of the map (pytorch_msssim.ssim(Y, X, data_range=1) by definition). loss3_dev [3] f32 = loss,
 * mse, ssim. With their pointers non-NULL also the gradients: gfeat_dev [n][ldg] (first 1,568
 * columns; ldg >= 1568) = dL/dfeat, what mz_stem_backward takes; dw_dec_dev [32][3][2][2],
 * db_dec_dev [3] (overwritten). ws_dev: mz_cae_workspace_floats(n) floats. Y stays on chip; sums
 * over samples run in a fixed order (no atomics). Refused (nothing launched), by both entry
 * points: a NULL required pointer, n < 1 or n > 4,194,304 (2^22: the workspace size stays an int;
 * mz_cae_workspace_floats returns 0 outside that range), ld or ldg < 1568, alpha outside [0, 1]. */
int mz_cae_loss(const uint32_t* bits_dev, const float* feat_dev, int32_t ld, int32_t n,
                const float* dec_w_dev, const float* dec_b_dev, float alpha, float* loss3_dev,
                float* gfeat_dev, int32_t ldg, float* dw_dec_dev, float* db_dec_dev, float* ws_dev,
                void* stream);
int mz_cae_workspace_floats(int32_t n);

/* The learner's parameter update: grad.clamp_(-clamp, clamp) on every parameter, then one
 * torch.optim.AdamW step (dqn_agent.py:152-157, ddqn_agent.py:148-152: AdamW(lr) with the
 * defaults betas (0.9, 0.999), eps 1e-8, weight_decay 1e-2 — the eager single-tensor formula)
 * over a flat f32 parameter buffer param_dev with its moment buffers exp_avg_dev /
 * exp_avg_sq_dev (same length, 16-byte aligned). Gradients come as nseg (<= 16) device segments:
 * grads_dev[k] (host array of device pointers, each 16-byte aligned) holds the gradient of flat
 * elements [sum(seg_len[:k]), sum(seg_len[:k+1])), seg_len[k] a multiple of 4; each is scaled by
 * grad_scale before the clamp (1/N after an all-reduce sum) and, if write_grad, written back
 * clamped. lr_dev: f32 learning rate on the device (the cosine schedule writes it); step_dev:
 * f32 step counter on the device, incremented by this call before the bias corrections (so a
 * captured HIP graph advances it on every replay). One launch over every parameter. */
/* nn.LeakyReLU(slope) in place on n bf16 values (the acting head's hidden layers, dqn_agent.py
 * :52-57): x > 0 ? x : x * slope in f32, rounded to nearest even — torch's leaky_relu_ on bf16
 * element for element. n a multiple of 8, x_dev 16-byte aligned. */
int mz_leaky_relu_bf16(uint16_t* x_dev, int64_t n, float slope, void* stream);

/* Column sums out_dev[c] = sum_{r < n} g_dev[r * ld + c], c < m, f32: the Linear bias gradient
 * db = dY^T 1 of the learner updates (the bias term of optimize_model's backward,
 * dqn_agent.py:150 / ppo_agent.py:235). m and ld multiples of 4, buffers 16-byte aligned;
 * fixed summation order (deterministic). */
int mz_colsum_f32(const float* g_dev, int32_t n, int32_t m, int32_t ld, float* out_dev,
                  void* stream);

/* One learner update's replay sample (ReplayMemory.sample, replay_memory.py:17-18, drawn as
 * indices on the device): rows idx_dev[i] (i < b, int64, clamped into [0, capacity)) of the state
 * arrays obs6 f32 [capacity][6] / window bits int32 [capacity][22] and of the next-state arrays
 * go to rows i and b + i of out_s6_dev f32 [2b][6] / out_sw_dev int32 [2b][22] (state rows, then
 * next-state rows), actions int64 and rewards f32 to out_a_dev / out_r_dev [b]. */
int mz_replay_gather(const int64_t* idx_dev, int32_t b, int64_t capacity,
                     const float* s6_dev, const int32_t* sw_dev, const int64_t* a_dev,
                     const float* r_dev, const float* s6n_dev, const int32_t* swn_dev,
                     float* out_s6_dev,
                     int32_t* out_sw_dev, int64_t* out_a_dev, float* out_r_dev, void* stream);

/* The PPO clipped surrogate with the reference's [b, b] broadcast (ppo_agent.py:188-197, clip
 * 0.3 there): for every column i, part_dev[i] = sum_j min(r a_i, clamp(r, 1-clip, 1+clip) a_i)
 * and dsum_dev[i] = sum_j r * w with r = exp(lp_new[i] - lp_old[j]) and w torch's gradient
 * routing through min / clamp (1/2 + 1/2 [inside] on ties, 1 where r a_i is the smaller, [inside]
 * otherwise). The loss is sum(part) / b^2 and dL/dlp_new[i] = a_i dsum[i] / b^2. All f32 [b]. */
int mz_pair_surrogate(const float* lp_new_dev, const float* lp_old_dev, const float* adv_dev,
                      int32_t b, float clip, float* part_dev, float* dsum_dev, void* stream);

/* The DQN/DDQN optimizer step (dqn_agent.py:152-157, ddqn_agent.py:148-152: grad.clamp_(-c, c)
 * per parameter, then torch.optim.AdamW) as one launch over a flat f32 parameter buffer whose
 * segment k (length seg_len[k], a multiple of 4) has its gradient at grads_dev[k] (host array of
 * nseg <= 16 device pointers). lr_dev: device f32 learning rate. step_dev: device f32 [1], the
 * step count, advanced by one by the call itself on `stream` (a one-thread launch behind the
 * update: a captured graph advances it per replay). write_grad: store the clamped,
 * grad_scale-scaled gradient back (clamp_ in place). */
int mz_adamw_flat(float* param_dev, float* exp_avg_dev, float* exp_avg_sq_dev,
                  const float* const* grads_dev, const int64_t* seg_len, int32_t nseg,
                  const float* lr_dev, float* step_dev, double beta1, double beta2, double eps,
                  double weight_decay, float clamp, float grad_scale, int32_t write_grad,
                  void* stream);

/* Set the per-instance algorithm ids used by regeneration (BaseMazeEnv.ALGORITHM is global in
 * the reference, base_maze_env.py:17,60-64; here it is per instance). algo_dev [B] or NULL. */
int mz_set_algorithm(mz_handle* h, const uint8_t* algo_dev, int32_t algo_all, void* stream);

/* Per-instance maze metadata into meta_dev [B][6] int32: N, start r, start c, goal r, goal c,
 * max_steps (the attributes maze_shape/_start_pos/_target_location/max_steps_taken). */
int mz_get_meta(mz_handle* h, int32_t* meta_dev, void* stream);

/* PPO discounted returns (ppo_agent.py:170-179) for n episodes on the device: episode k is row
 * rows_dev[k] of rew_dev (float64, leading dim ld) with length lens_dev[k]; out_dev[k*ldo + t] =
 * float32(sum_j gamma^j r[t+j]) accumulated backwards in float64 like the reference's loop. */
int mz_discounted_returns(const double* rew_dev, int32_t ld, const int32_t* rows_dev,
                          const int32_t* lens_dev, int32_t n, double gamma, float* out_dev,
                          int32_t ldo, void* stream);

/* McClendon difficulty of a maze (host computation, synchronous): ComplexityEvaluation(maze,
 * start, goal).difficulty_of_maze() (maze_complexity_evaluation.py:38-329) for a euclidean grid
 * (toroidal mazes: pass the bordered (N+2) grid, as gen_maze_no_border does, :37-56).
 * Used by get_maze_difficulty (base_maze_env.py:99-105) and best-of-6 generation (:78-97). */
int mz_difficulty(const uint8_t* grid_host, int32_t h, int32_t w, int32_t sr, int32_t sc,
                  int32_t gr, int32_t gc, double* out_host);

/* McClendon difficulty and complexity together (complexity_of_maze :311-317 = log of the sum of
 * the branch complexities; difficulty as mz_difficulty). Either output may be NULL. Host,
 * synchronous. */
int mz_maze_complexity(const uint8_t* grid_host, int32_t h, int32_t w, int32_t sr, int32_t sc,
                       int32_t gr, int32_t gc, double* difficulty_out, double* complexity_out);

/* McClendon difficulty of resident mazes on the GPU, one workgroup per maze (replaces the
 * per-maze host ComplexityEvaluation(...).difficulty_of_maze() calls of best-of-6 generation,
 * base_maze_env.py:84-95, maze_complexity_evaluation.py:38-329). For the listed instances
 * (env_ids_dev NULL = all B): out_dev [n][2] float64 = {prod, sum}, the reference's product
 * prod_b (C_b + 1) * C_0 and sum sum_b C_b + C_0 BEFORE math.log (the caller takes the log with
 * the C library, as the reference: difficulty = log(prod), complexity = log(sum)), each hallway
 * summed in the order networkx's subgraph view iterates its CPython set (bit-exact with the
 * reference); a toroidal handle's maze is scored as its bordered (N + 2)^2 maze with start / goal
 * shifted by +1, as the reference scores it (off_policy_trainer.py:194-196). status_dev [n]
 * int32: 0 ok, 1 not a perfect maze (cycles / unreachable squares), 2 outside the kernel's cases
 * (open border squares, straight goal square, all solution points junctions, more points than
 * the LDS plan holds, a hallway of more than 63 view nodes), 3 invalid (start == goal, bad id,
 * log domain) — the caller computes every nonzero-status maze with mz_difficulty (toroidal: on
 * the bordered grid). Asynchronous on `stream`. Returns MZ_EINVAL_SHAPE when the evaluated grid's
 * pitch exceeds the kernel's LDS plan (odd pitches: P > 91; toroidal P > 89 — the bordered grid
 * is P + 2; tests/test_abi.py derives both limits from the plan). */
int mz_difficulty_batch(mz_handle* h, const int32_t* env_ids_dev, int32_t n, double* out_dev,
                        int32_t* status_dev, void* stream);
/* The order-free McClendon screen (csrc/mz_screen.hip; the best-of-C selection's first stage) of
 * the listed euclidean instances (NULL = all B): out_dev [n][2] float64 = {prod, e} — the product
 * prod_b (C_b + 1) * C_0 of maze_complexity_evaluation.py:319-329 summed in an order of its own,
 * and a rigorous bound e on |prod_ref - prod| / prod for the reference's evaluation order (which
 * mz_difficulty_batch reproduces); status_dev [n] int32: 0 ok, 2 declined (not a perfect maze on
 * the odd lattice with a dead-end goal, or beyond the LDS plan). One wave per maze. */
int mz_screen_batch(mz_handle* h, const int32_t* env_ids_dev, int32_t n, double* out_dev,
                    int32_t* status_dev, void* stream);

/* The reference's maze-metric suite (MetricsCalculator, metrics_calculator.py:11-133, as used by
 * generation_algos_metrics_evaluations.py:33-45) for the listed euclidean instances (NULL = all B),
 * computed on the GPU from the instances' mazes: out_dev [n][6] float64 = L, DE, D, AC, FDE, BDE
 * of the solution path (calculate_L / calculate_DE / calculate_D / calculate_DE_sub). */
int mz_maze_metrics(mz_handle* h, const int32_t* env_ids_dev, int32_t n, double* out_dev,
                    void* stream);

/* Synchronous host snapshots for the single-env drop-in classes. */
int mz_query(mz_handle* h, int32_t env, mz_env_info* info_host);
int mz_get_grid(mz_handle* h, int32_t env, uint8_t* grid_host /* [n][n] */);

/* Page-locked host memory mapped into the device's address space (hipHostMalloc, mapped +
 * coherent): kernels read and write it through *dev_out. The single-env drop-ins keep their
 * action and per-step outputs there, so one reference step() (base_maze_env.py:163-210) is one
 * launch + one stream synchronisation, with no device<->host copies. Free with mz_host_free. */
int mz_host_alloc(uint64_t bytes, int32_t device, void** host_out, void** dev_out);
int mz_host_free(void* host);

/* ---- Vectorised trainer bookkeeping (mazerl/trainers/vector_trainer.py; the training loop of
 * NeuralOffPolicyTrainer.train, lib/trainers/off_policy_trainer.py:144-225, over n instances).
 * The loop waits once per vector step for the greedy-row count; these calls keep the launches
 * behind that wait few. */

/* After a vector step: steps_done += 1, = 0 where terminated (off_policy_trainer.py:192, per
 * instance); eps_out = eps_final + (eps_start - eps_final) * exp(-steps_done / eps_decay) in f32
 * (dqn_agent.py:118-119 calculate_epsilon, as the learner's torch expression rounds it);
 * wins += #terminated, episodes += #(terminated | truncated) (int64 device counters, nullable);
 * and the greedy-row list of the NEXT fused act (seed, counter, eps_out): rows_dev / count_dev as
 * mz_greedy_rows. scratch_dev: int32 [ceil(n / 1024)]. */
int mz_trainer_tick(const uint8_t* term_dev, const uint8_t* trunc_dev, float* steps_done_dev,
                    double eps_start, double eps_final, double eps_decay, float* eps_out_dev,
                    int64_t* wins_dev, int64_t* episodes_dev, uint64_t seed, uint64_t counter,
                    int32_t n, int32_t* scratch_dev, int32_t* rows_dev, int32_t* count_dev,
                    void* stream);

/* greedy_dev[rows_dev[i]] = argmax_a q_dev[i][a] (first maximum, torch.argmax) for
 * i < min(*count_dev, m): the acting forward's bf16 Q rows [m][ldq] (dqn_agent.py:113-116
 * `.max(1)[1]`) scattered to the listed instances; the list length is read on the device. */
int mz_greedy_scatter(const uint16_t* q_dev, int32_t ldq, const int32_t* rows_dev,
                      const int32_t* count_dev, int32_t m, int64_t* greedy_dev, void* stream);

/* bf16 copy of the acting head's three Linear layers (dqn_agent.py:47-57 / ddqn_agent.py:40-52
 * fc): w_l f32 [out_l][in_l] -> dw_l bf16 (round to nearest even, torch's .to(bfloat16)); fc1's
 * first conv_out columns permuted from torch's channel-major flatten (c * Q + q, Q = conv_out /
 * conv_ch) to the fused stem's position-major order (q * conv_ch + c), rows padded with zeros to
 * ld0 (in0 <= 2048); biases b_l -> db_l. One launch. */
int mz_head_bf16(const float* w0, const float* b0, const float* w1, const float* b1,
                 const float* w2, const float* b2, int32_t out0, int32_t in0, int32_t out1,
                 int32_t in1, int32_t out2, int32_t in2, int32_t ld0, int32_t conv_out,
                 int32_t conv_ch, uint16_t* dw0, uint16_t* db0, uint16_t* dw1, uint16_t* db1,
                 uint16_t* dw2, uint16_t* db2, void* stream);

/* Replay ring push (lib/replay_memory.py:14 push, a vector step at once): ring rows ptr ..
 * ptr + n - 1 (mod capacity) of s6 f32 [C][obs_dim], sw int32 [C][window_words], a int64 [C]
 * (from int32 actions), r f32 [C], s6n, swn <- the n source rows; a NULL source leaves its array
 * untouched (the state half can be written before the env step overwrites the observation). */
int mz_replay_push(int32_t n, int64_t capacity, int64_t ptr, const float* obs6_src,
                   const int32_t* bits_src, const int32_t* act_src, const float* rew_src,
                   const float* obs6n_src, const int32_t* bitsn_src, float* s6_dev,
                   int32_t* sw_dev, int64_t* a_dev, float* r_dev, float* s6n_dev,
                   int32_t* swn_dev, int32_t obs_dim, int32_t window_words, void* stream);

/* n uniform replay rows (random.sample of replay_memory.py:17, with replacement) among the newest
 * n_avail ring rows ending at row `newest`: out_dev[i] = (newest - floor(u_i * n_avail)) mod
 * capacity, u_i a 53-bit uniform from Philox(seed, i, counter). */
int mz_replay_sample_idx(uint64_t seed, uint64_t counter, int64_t newest, int64_t n_avail,
                         int64_t capacity, int64_t* out_dev, int32_t n, void* stream);

/* Q-learning loss of optimize_model (dqn_agent.py:129-147, ddqn_agent.py:121-143) from the nets'
 * f32 output rows: for i < b, Q(s,a) = q_dev[i][action_dev[i]]; V(s') = q_tgt_dev[i][argmax_a
 * q_next_dev[i][a]] (DDQN; first maximum) or max_a q_tgt_dev[i][a] (DQN: q_next_dev NULL);
 * diff_dev[i] = Q(s,a) - (V(s') * gamma + reward_dev[i]) — no terminal masking (the reference
 * bootstraps terminal transitions); *loss_dev = mse_loss (mean) = sum diff^2 / b.
 * Row strides ldq / ldn / ldt in floats (>= 4). One workgroup. */
int mz_q_loss(const float* q_dev, int32_t ldq, const float* q_next_dev, int32_t ldn,
              const float* q_tgt_dev, int32_t ldt, const int64_t* action_dev,
              const float* reward_dev, double gamma, int32_t b, float* loss_dev, float* diff_dev,
              void* stream);

/* Its gradient w.r.t. q rows [rows][4] (contiguous; rows >= b — DDQN's stacked s' rows — get 0):
 * dq[i][action[i]] = diff[i] * (2 / b) * (*grad_dev), 0 elsewhere. */
int mz_q_loss_backward(const float* grad_dev, const float* diff_dev, const int64_t* action_dev,
                       int32_t b, int32_t rows, float* dq_dev, void* stream);

/* The Q head and the loss of optimize_model in one launch, from the second hidden layer's
 * pre-activation rows z2 (f32, row stride lds / ldt floats, `hidden` columns, a multiple of 4) of
 * the source and the target net: h = act(z2) (act 0: LeakyReLU(0.01), DQN; 1: ReLU, DDQN),
 * q = W3 h + b3 (fc3: W3 [4][hidden], b3 [4]); with `stacked` the source rows are DDQN's [s; s']
 * (2b rows: V(s') = q_t[argmax q_s(s')], first maximum), else b rows and V(s') = max q_t; then
 * diff_dev / *loss_dev exactly as mz_q_loss (dqn_agent.py:129-147, ddqn_agent.py:121-143).
 * part_dev: mz_head_loss_workspace_floats(b) floats (one per concurrently running call);
 * ticket_dev: unused since round 5 (the per-workgroup partials are summed by a second launch on
 * `stream`), may be NULL. Replaces the activation, fc3 and loss launches of both nets. */
int mz_head_loss_workspace_floats(int32_t b);
int mz_head_loss(const float* z2s_dev, int32_t lds, const float* w3s_dev, const float* b3s_dev,
                 const float* z2t_dev, int32_t ldt, const float* w3t_dev, const float* b3t_dev,
                 int32_t hidden, int32_t act, int32_t stacked, const int64_t* action_dev,
                 const float* reward_dev, double gamma, int32_t b, float* part_dev,
                 uint32_t* ticket_dev, float* loss_dev, float* diff_dev, void* stream);

/* Its backward through fc3 and the activation for the source rows i < b: dz2_dev[i][j] =
 * act'(z2[i][j]) * g_i W3[a_i][j], g_i = diff[i] * (2 / b) * (*grad_dev) (rows >= b untouched),
 * and per block of rows the partial sums of dW3 (row-major [4][hidden]) and db3 [4] into part_dev
 * ([blocks][4 hidden + 4], mz_head_loss_backward_workspace_floats floats): their column sums
 * (mz_colsum_f32 over blocks rows of 4 hidden + 4) are fc3's weight and bias gradients. */
int mz_head_loss_backward_workspace_floats(int32_t b, int32_t hidden);
int mz_head_loss_backward(const float* grad_dev, const float* diff_dev, const int64_t* action_dev,
                          int32_t b, const float* z2s_dev, int32_t lds, const float* w3s_dev,
                          int32_t hidden, int32_t act, float* dz2_dev, int32_t ldd,
                          float* part_dev, void* stream);

/* PPO's optimizer step (ppo_agent.py:232-236, optimize_model): clip_grad_norm_(params, max_norm)
 * (coef = min(max_norm / (||g||_2 + 1e-6), 1) over every gradient, the gradients scaled in place;
 * max_norm <= 0: no clipping), then AdamW (torch's defaults: betas, eps, weight_decay given) with
 * a learning rate per parameter group — segment k of the flat buffer (mz_adamw_flat's layout)
 * uses lr_dev[seg_group[k]] (ppo_agent.py's three groups: actor lr, critic lr, their mean for
 * the conv stem). step_dev is incremented on the device (capturable). scratch_dev: >= 513
 * floats. Three launches. */
int mz_adamw_groups(float* param_dev, float* exp_avg_dev, float* exp_avg_sq_dev,
                    const float* const* grads_dev, const int64_t* seg_len,
                    const int32_t* seg_group, int32_t nseg, const float* lr_dev, float* step_dev,
                    double beta1, double beta2, double eps, double weight_decay, float max_norm,
                    float* scratch_dev, void* stream);

/* ---- Config 5's PPO rollout on the device (VectorPPOTrainer; no host round trip per step) ----
 * B instances, per-instance episode records [B][L] at the instance's own step index t_dev[i]
 * (L > the longest possible episode). Replaces, per instance, PPOAgent.do_episode's loop
 * (agents/ppo_agent.py:143-169) and PPOTrainer.train's Buffer.add (lib/trainers/ppo_trainer.py
 * :15-46, :66-67). */

/* ActorCriticNet.act (ppo_agent.py:55-68) from the f32 actor logits [B][ldl] and critic values
 * [B] (stride ldv): softmax as torch forms it for a 4-wide row, one draw per instance (inverse
 * CDF of a Philox uniform: P(a) = softmax(logits)[a], torch.multinomial's distribution), the
 * draw's log-prob log(p[a]); records obs6, the 22 window-bit words, action (int64), log-prob and
 * value at [i][t_dev[i]] (do_episode's appends, :150-156) and writes the action to act_out_dev
 * (int32, mz_step's input). The draw is a function of (seed, counter, i) alone. Where t_dev[i] is
 * outside [0, L) the instance is skipped: nothing is recorded, no draw is made and act_out_dev[i]
 * is left as it was (unlike mz_rf_act, which still draws and writes the action); mz_ppo_scan
 * keeps t_dev inside, so the caller never steps with such an entry. */
int mz_ppo_act(const float* logits_dev, int32_t ldl, const float* value_dev, int32_t ldv,
               const float* obs6_dev, const uint32_t* bits_dev, int32_t B, int32_t L, uint64_t seed,
               uint64_t counter, const int32_t* t_dev, float* rec_s6_dev, uint32_t* rec_w_dev,
               int64_t* rec_a_dev, float* rec_lp_dev, float* rec_v_dev, int32_t* act_out_dev,
               void* stream);

/* After mz_step: the float64 reward at [i][t_dev[i]] (rewards.append, :158), t_dev[i] += 1, and
 * for every instance whose step ended (terminated | truncated, :161): t_dev[i] = 0, stats_dev
 * [0] += 1 (episodes), [1] += terminated (wins), and — for episodes of >= 2 steps (a 1-step
 * episode's returns are NaN: torch.std of one element; counted in stats_dev[2] instead) — an
 * entry in the finished list (instance fin_id, pool row fin_off, length fin_len; instance order)
 * placed after the pool's current *pool_fill_dev rows; *pool_fill_dev and the monotonic
 * *pool_total_dev grow by the listed rows. stats_dev[3] counts unfinished episodes that reached
 * L steps (their records would leave the [B][L] buffers; t_dev stays at L - 1): the caller sizes
 * L past every max_steps + 1 and treats a nonzero count as an error. stats_dev is int64[4].
 * One workgroup. */
int mz_ppo_scan(const double* reward64_dev, const uint8_t* term_dev, const uint8_t* trunc_dev,
                int32_t B, int32_t L, int32_t* t_dev, double* rec_r_dev, int32_t* fin_id_dev,
                int64_t* fin_off_dev, int32_t* fin_len_dev, int32_t* fin_count_dev,
                int64_t* pool_fill_dev, int64_t* pool_total_dev, int64_t* stats_dev,
                void* stream);

/* For every listed episode: calculate_returns (ppo_agent.py:171-181: acc = r + acc * gamma
 * backwards in float64, float32, (R - mean) / std, unbiased std) and calculate_advantages
 * (:183-186: A = R - V, (A - mean) / (std + 1e-8)) — sums in float64, mean / std rounded to
 * float32 — and the episode's rows (obs6, window bits, action, log-prob, advantage, return)
 * into the pool columns at its rows (rows past `capacity` are not written: the caller checks
 * *pool_fill_dev <= capacity). One workgroup per episode. */
int mz_ppo_finish(const double* rec_r_dev, const float* rec_s6_dev, const uint32_t* rec_w_dev,
                  const int64_t* rec_a_dev, const float* rec_lp_dev, const float* rec_v_dev,
                  int32_t B, int32_t L, const int32_t* fin_id_dev, const int64_t* fin_off_dev,
                  const int32_t* fin_len_dev, const int32_t* fin_count_dev, double gamma,
                  int64_t capacity, float* pool_s6_dev, uint32_t* pool_w_dev, int64_t* pool_a_dev,
                  float* pool_lp_dev, float* pool_adv_dev, float* pool_ret_dev, void* stream);

/* The PPO minibatch loss in three launches (ppo_agent.py:188-203 through ActorCriticNet.evaluate,
 * :55-66, and optimize_model's total = policy + 0.5 value, :222-224): for b rows of 4 action
 * logits (row stride ldl), value (stride ldv), action, old log-prob, advantage, return and the
 * entropy coefficient (device scalar): softmax, the action's log_softmax, entropy
 * -sum p log(p + 1e-8), the clipped surrogate over the reference's [b, b] ratio broadcast
 * (mz_pair_surrogate), total = -(surrogate + coef * mean entropy) + 0.5 * mean((v - ret)^2) into
 * loss_dev[0], and d total / d logits (dlogits_dev, row stride ldg) and d total / d value
 * (dvalue_dev, stride ldvg). scratch_dev: 12 b floats. Sums in a fixed order (deterministic). */
int mz_ppo_head_loss(const float* logits_dev, int32_t ldl, const float* value_dev, int32_t ldv,
                     const int64_t* action_dev, const float* lp_old_dev, const float* adv_dev,
                     const float* ret_dev, const float* coef_dev, int32_t b, float clip,
                     float* scratch_dev, float* loss_dev, float* dlogits_dev, int32_t ldg,
                     float* dvalue_dev, int32_t ldvg, void* stream);

/* ---- REINFORCE on the device (VectorReinforceTrainer) ----------------------------------------
 * RFAgent (agents/rf_agent.py:51-129) under ValueBasedTrainer.train (lib/trainers/
 * value_based_trainer.py:25-92), per instance. The [B][L] episode records, mz_ppo_scan and the
 * update pool are the PPO rollout's; these three entry points are REINFORCE's own arithmetic.
 * Each refuses a null pointer, B, L or b < 0, a temperature that is not > 0 and a row stride < 4
 * with MZ_EINVAL before any GPU call; B == 0 / b == 0 is a no-op. */

/* select_action (:73-86) from the f32 policy logits [B][ldl]: softmax(logits / temperature) as
 * torch forms it for a 4-wide row, one draw per instance (inverse CDF of a Philox uniform keyed
 * by (seed, counter, instance): P(a) = softmax(logits / temperature)[a], torch.multinomial's
 * distribution); records obs6, the 22 window-bit words and the action (int64) at
 * [i][t_dev[i]] where 0 <= t_dev[i] < L (nothing is recorded otherwise; the draw happens either
 * way) and writes the action to act_out_dev (int32, mz_step's input). No log-prob and no value
 * are recorded: the update recomputes the forward. */
int mz_rf_act(const float* logits_dev, int32_t ldl, float temperature, const float* obs6_dev,
              const uint32_t* bits_dev, int32_t B, int32_t L, uint64_t seed, uint64_t counter,
              const int32_t* t_dev, float* rec_s6_dev, uint32_t* rec_w_dev, int64_t* rec_a_dev,
              int32_t* act_out_dev, void* stream);

/* After mz_ppo_scan, for every listed episode: get_returns (:88-99: R = r + gamma R backwards in
 * float64, float32, (R - mean) / (std + 1e-6), unbiased std) and optimize_model's baseline
 * (:109-110: adv = R - mean(R)) -- sums in float64, mean / std rounded to float32 -- and the
 * episode's rows (obs6, window bits, action, adv, the episode's length on every row) into the
 * pool columns at its rows; *episodes_dev += the episodes pooled. Rows past `capacity` are not
 * written (the caller checks *pool_fill_dev <= capacity). One workgroup per episode. */
int mz_rf_finish(const double* rec_r_dev, const float* rec_s6_dev, const uint32_t* rec_w_dev,
                 const int64_t* rec_a_dev, int32_t B, int32_t L, const int32_t* fin_id_dev,
                 const int64_t* fin_off_dev, const int32_t* fin_len_dev,
                 const int32_t* fin_count_dev, double gamma, int64_t capacity, float* pool_s6_dev,
                 uint32_t* pool_w_dev, int64_t* pool_a_dev, float* pool_adv_dev,
                 int32_t* pool_len_dev, int32_t* episodes_dev, void* stream);

/* optimize_model's loss (:101-118) over b pool rows of 4 logits (row stride ldl), as the mean
 * over the E = *episodes_dev pooled episodes of the per-episode loss: with z = x / temperature,
 * p = softmax(z), q = p + 1e-10, l = log q and T = len_dev[row],
 *   f = (1 / E) (-adv l_a - (entropy_coef / T) (-sum_k q_k l_k))
 * loss_dev[0] = sum of f over the rows (float64 sum in a fixed order, stored as f32) and
 * dlogits_dev (row stride ldg) = d f / d x, in one launch. With E = 1 and the rows of one whole
 * episode this is the reference's loss. */
int mz_rf_head_loss(const float* logits_dev, int32_t ldl, const int64_t* action_dev,
                    const float* adv_dev, const int32_t* len_dev, const int32_t* episodes_dev,
                    int32_t b, float temperature, float entropy_coef, float* loss_dev,
                    float* dlogits_dev, int32_t ldg, void* stream);

/* ---- The recurrent DQN on the device (VectorRecurrentDQNTrainer) -----------------------------
 * agents/lstm_dqn_agent.py: nn.LSTMCell(6, 32) + nn.Linear(32, 4) over obs6, trained from whole
 * episodes. params_dev is a HOST array of six device pointers in state_dict order
 * (lstm_cell.weight_ih [128][6], weight_hh [128][32], bias_ih [128], bias_hh [128], fc.weight
 * [4][32], fc.bias [4]; torch's layouts, gate order i, f, g, o). A gate pre-activation is
 * (bias_ih + bias_hh), then the 6 input terms, then the 32 recurrent terms, one fmaf each; a q
 * value is fc.bias then 32 fmaf. The reward records [B][L] (float64), t_dev and the finished
 * episodes' list are mz_ppo_scan's. Every entry point refuses a null pointer, B < 1, E < 1,
 * hidden != 32 and capacity < E with MZ_EINVAL before any GPU call. */

/* One acting step of B instances: from (h, c) (h_dev / c_dev, [32][B] f32, updated in place; taken
 * as zero where t_dev[i] == 0) and x = obs6_dev[i] the cell and the head, then the action: one
 * Philox draw per instance keyed by (seed, counter, instance) — word 0 (24 bits) < epsilon
 * explores, and the action is then floor(word 1 * explore_actions / 2^32); else the first argmax
 * of q. Where 0 <= t_dev[i] < L, x goes to rec_x_dev[i][t] ([B][L + 1][6]) and the action to
 * rec_a_dev[i][t] ([B][L] int32); where t_dev[i] is outside, the action is still produced but
 * nothing is recorded and (h, c) stay as they were. L == 0 is the evaluation mode: no records
 * (rec pointers may be NULL) and every instance's state advances. act_out_dev: int32 [B];
 * q_out_dev: f32 [B][4] or NULL. */
int mz_drqn_act(const float* const* params_dev, int32_t hidden, const float* obs6_dev, int32_t B,
                int32_t L, float epsilon, int32_t explore_actions, uint64_t seed, uint64_t counter,
                const int32_t* t_dev, float* h_dev, float* c_dev, float* rec_x_dev,
                int32_t* rec_a_dev, int32_t* act_out_dev, float* q_out_dev, void* stream);

/* After mz_ppo_scan, for its k-th listed episode (instance i, n steps): obs6_dev[i] (the
 * observation after the last step) into rec_x_dev[i][n], and the episode into ring slot
 * (head + k) mod capacity: n + 1 rows of 8 words (x[6] f32, action i32, reward f32 = (float) of
 * the float64 record; row n holds x_n only), mem_len_dev[slot] = n, mem_term_dev[slot] =
 * term_dev[i] != 0. Then ring_dev (int64: head, count) moves on by the listed episodes. With
 * more listed episodes than slots the last `capacity` of them stay. mz_ppo_scan does not list
 * 1-step episodes, so none reaches the memory. */
int mz_drqn_store(const float* obs6_dev, const uint8_t* term_dev, int32_t B, int32_t L,
                  const int32_t* fin_id_dev, const int32_t* fin_len_dev,
                  const int32_t* fin_count_dev, float* rec_x_dev, const int32_t* rec_a_dev,
                  const double* rec_r_dev, int64_t capacity, uint32_t* mem_dev,
                  int32_t* mem_len_dev, int32_t* mem_term_dev, int64_t* ring_dev, void* stream);

/* E distinct slots of the filled part of the ring, every E-subset equally likely (Philox keyed by
 * (seed, counter)), and the batch directory: dir_slot / dir_len [E] int32, dir_off [E] int64 =
 * the exclusive scan of (len + 1) (an episode's first row in the update's row buffers), dir_tot
 * int64 [2] = (rows = sum (len + 1), steps = sum len). `filled` is the caller's knowledge of the
 * ring's count (the device's count is at least that); E > filled is refused. */
int mz_drqn_sample(uint64_t seed, uint64_t counter, int32_t E, int32_t L, int64_t capacity,
                   int64_t filled, const int64_t* ring_dev, const int32_t* mem_len_dev,
                   int32_t* dir_slot_dev, int32_t* dir_len_dev, int64_t* dir_off_dev,
                   int64_t* dir_tot_dev, void* stream);

/* The net unrolled from zero state over each directory episode, one wave per episode. Row buffers
 * hold E (L + 1) rows; episode e uses rows dir_off[e] .. dir_off[e] + len (the last is a guard
 * row only the target writes). target != 0: x_0 .. x_n, qmax_dev[row] = max_a Q'_t (the other
 * outputs may be NULL). target == 0: x_0 .. x_{n-1}; reads qmax_dev; per step stash_dev[row][192]
 * (gates i, f, g, o after their nonlinearity, c, h), qa_dev = Q_t[a_t], y_dev = r_t + gamma
 * qmax[t + 1] (r_t alone at the last step of a terminated episode), d_dev = 2 (Q_t[a_t] - y_t) /
 * steps; ep_loss_dev[e] (float64) = the episode's sum of squared residuals in time order. */
int mz_drqn_seq_forward(const float* const* params_dev, int32_t hidden, int32_t target, int32_t E,
                        int32_t L, int64_t capacity, float gamma, const uint32_t* mem_dev,
                        const int32_t* mem_term_dev, const int32_t* dir_slot_dev,
                        const int32_t* dir_len_dev, const int64_t* dir_off_dev,
                        const int64_t* dir_tot_dev, float* qmax_dev, float* stash_dev,
                        float* qa_dev, float* y_dev, float* d_dev, double* ep_loss_dev,
                        void* stream);

/* Back-propagation through time of loss = sum of squared residuals / steps from the source
 * forward's stash and d_dev: one wave per episode writes its gradient to gpart_dev [E][5252] (flat
 * state_dict order), then per parameter the partials are summed over the episodes in index order
 * (float64, rounded once) into grads_dev (a HOST array of six device pointers, state_dict order;
 * overwritten, not accumulated) and loss_dev[0] = sum of ep_loss / steps. No atomics: the same
 * inputs give the same bits. */
int mz_drqn_seq_backward(const float* const* params_dev, int32_t hidden, int32_t E, int32_t L,
                         int64_t capacity, const uint32_t* mem_dev, const int32_t* dir_slot_dev,
                         const int32_t* dir_len_dev, const int64_t* dir_off_dev,
                         const int64_t* dir_tot_dev, const float* stash_dev, const float* d_dev,
                         const double* ep_loss_dev, float* gpart_dev, float* const* grads_dev,
                         float* loss_dev, void* stream);

/* ---- Replay windows with stored state and burn-in (VectorRecurrentDQNTrainer(window=T)) -------
 * An update trains on one window of T steps per sampled episode instead of the whole episode:
 * window j of an episode of n steps covers steps s = j T .. s + m - 1, m = min(T, n - s),
 * j = 0 .. ceil(n / T) - 1. Both nets start at step b = max(0, s - K) (K = the burn-in, a multiple
 * of T) from the same state, snapshot b / T of the episode, or zero where b == 0 or no snapshots
 * are kept, and unroll k = s - b burn-in steps that carry no loss term and no gradient. A
 * snapshot is 64 f32 (h[32], c[32]): the state the instance held before it acted at step j T,
 * j >= 1; an episode has ceil(L / T) snapshot entries, entry 0 is never written. The accumulation
 * order of a step is the one stated above. Every entry point refuses a null pointer, T < 1, K < 0,
 * K % T != 0, hidden != 32, E < 1, B < 1, L < 1 and capacity < E with MZ_EINVAL before any GPU
 * call, as far as it has the argument. */

/* Before mz_drqn_act of the same vector step: where 0 < t_dev[i] < L and t_dev[i] % T == 0, column
 * i of h_dev / c_dev ([32][B]) goes to snap_rec_dev[i][t / T] ([B][ceil(L / T)][64]). */
int mz_drqn_snapshot(int32_t hidden, int32_t B, int32_t L, int32_t T, const int32_t* t_dev,
                     const float* h_dev, const float* c_dev, float* snap_rec_dev, void* stream);

/* After mz_ppo_scan and BEFORE mz_drqn_store (which advances ring_dev): snapshots 1 ..
 * ceil(n / T) - 1 of its k-th listed episode (instance i, n steps) from snap_rec_dev[i] into
 * mem_state_dev[(head + k) mod capacity] ([capacity][ceil(L / T)][64]), the slot mz_drqn_store
 * gives the episode; with more listed episodes than slots the last `capacity` stay. Nothing else
 * of mem_state_dev is written. */
int mz_drqn_snap_store(int32_t hidden, int32_t B, int32_t L, int32_t T, const int32_t* fin_id_dev,
                       const int32_t* fin_len_dev, const int32_t* fin_count_dev,
                       const float* snap_rec_dev, int64_t capacity, float* mem_state_dev,
                       const int64_t* ring_dev, void* stream);

/* mz_drqn_sample's E slots (the same draws for the same (seed, counter)), then for batch position
 * e one window j = floor(u32 ceil(n / T) / 2^32) from a Philox stream of its own keyed by (seed,
 * counter, e): windows are uniform within an episode, not over the memory. wdir_dev is int32
 * [5][E]: slot, n, b, k, m. win_off_dev [E] int64 = the exclusive scan of (m + 2): window e owns
 * rows win_off[e] (the entry state), + 1 .. + m (its training steps) and + m + 1 (the guard row)
 * of the update's row buffers, which hold E (min(T, L) + 2) rows whatever L and K are.
 * win_tot_dev int64 [2] = (rows, sum m). */
int mz_drqn_window_sample(uint64_t seed, uint64_t counter, int32_t hidden, int32_t E, int32_t L,
                          int32_t T, int32_t K, int64_t capacity, int64_t filled,
                          const int64_t* ring_dev, const int32_t* mem_len_dev, int32_t* wdir_dev,
                          int64_t* win_off_dev, int64_t* win_tot_dev, void* stream);

/* mz_drqn_seq_forward over the directory's windows, one wave per window, from mem_state_dev's
 * snapshots (NULL: zero state). target != 0: x_b .. x_{s+m}, qmax_dev[win_off + 1 + i] = max_a
 * Q'_{s+i}, i = 0 .. m. target == 0: x_b .. x_{s+m-1}; stash_dev[win_off][128 .. 191] = (c, h)
 * entering step s; per training step i at row win_off + 1 + i the stash, qa_dev, y_dev = r +
 * gamma qmax[row + 1] (r alone where s + i == n - 1 and the episode terminated), d_dev =
 * 2 (Q - y) / sum m; ep_loss_dev[e] = the window's sum of squared residuals. With T >= L and K == 0
 * these are mz_drqn_seq_forward's bits, one row further down. */
int mz_drqn_window_forward(const float* const* params_dev, int32_t hidden, int32_t target,
                           int32_t E, int32_t L, int32_t T, int32_t K, int64_t capacity,
                           float gamma, const uint32_t* mem_dev, const int32_t* mem_term_dev,
                           const float* mem_state_dev, const int32_t* wdir_dev,
                           const int64_t* win_off_dev, const int64_t* win_tot_dev, float* qmax_dev,
                           float* stash_dev, float* qa_dev, float* y_dev, float* d_dev,
                           double* ep_loss_dev, void* stream);

/* mz_drqn_seq_backward over the m training steps of each window (nothing flows into the burn-in
 * or the entry state): gpart_dev [E][5252], then grads_dev and loss_dev[0] = sum of ep_loss /
 * sum m, reduced in index order as there. */
int mz_drqn_window_backward(const float* const* params_dev, int32_t hidden, int32_t E, int32_t L,
                            int32_t T, int32_t K, int64_t capacity, const uint32_t* mem_dev,
                            const int32_t* wdir_dev, const int64_t* win_off_dev,
                            const int64_t* win_tot_dev, const float* stash_dev,
                            const float* d_dev, const double* ep_loss_dev, float* gpart_dev,
                            float* const* grads_dev, float* loss_dev, void* stream);

/* ---- Prioritized replay windows (VectorRecurrentDQNTrainer(window=T, priority_alpha=a)) --------
 * Every window (slot, j) of the replay ring carries a mass: an unsigned 32-bit fixed-point priority
 * with 20 fractional bits, 0 = no such window. mem_prio_dev is uint32 [capacity][W], W =
 * ceil(L / T); mem_psum_dev uint64 [capacity] holds each slot's sum of masses; prio_max_dev uint32
 * [1] the largest mass an update has written (the caller starts it at 2^20, priority 1). Every sum
 * over masses is an exact 64-bit integer, so no result below depends on a reduction's order and the
 * sampler equals a host model bit for bit; no float atomics are used. Every entry point refuses a
 * null pointer, T < 1, hidden != 32, E < 1, B < 1, L < 1, capacity < 1, K < 0, K % T != 0, alpha
 * < 0, beta < 0, eta outside [0, 1], eps <= 0, a non-finite parameter, and capacity W E 2^30 >= 2^63
 * (the bound under which every product fits 64 bits; a store counts E = 1) with MZ_EINVAL before
 * any GPU call, as far as it has the argument. */

/* After mz_ppo_scan and BEFORE mz_drqn_store (it reads the head the store advances), by
 * mz_drqn_store's slot rule and validity tests: the k-th listed episode (n steps) gives entries
 * 0 .. ceil(n / T) - 1 of mem_prio_dev[(head + k) mod capacity] the mass prio_max_dev[0], the
 * slot's other entries 0, and mem_psum_dev[slot] = ceil(n / T) prio_max; with more listed episodes
 * than slots the last `capacity` stay. One workgroup per listed episode. */
int mz_drqn_prio_store(int32_t hidden, int32_t B, int32_t L, int32_t T, const int32_t* fin_id_dev,
                       const int32_t* fin_len_dev, const int32_t* fin_count_dev, int64_t capacity,
                       uint32_t* mem_prio_dev, uint64_t* mem_psum_dev, const uint32_t* prio_max_dev,
                       const int64_t* ring_dev, void* stream);

/* In mz_drqn_window_sample's place: E windows with replacement, in proportion to their mass,
 * stratified. S = the sum of mem_psum_dev over slots 0 .. capacity - 1; batch position e draws
 * t = lo + mulhi64(r, hi - lo), lo = floor(e S / E), hi = floor((e + 1) S / E), r = (r0 << 32) | r1
 * of a Philox stream of its own keyed by (seed, counter, e), and takes the window (slot, j) with
 * prefix <= t < prefix + mass, the prefix running slot-major, j-minor over all masses. From j:
 * s = j T, b = max(0, s - K), k = s - b, m = min(T, n - s); wdir_dev, win_off_dev and win_tot_dev
 * are mz_drqn_window_sample's, so mz_drqn_window_forward / _backward run on them as they are. Two
 * positions may hold the same window. isw_dev[e] = (float) pow((double) M_min / M_e, beta), M_e the
 * sampled window's mass and M_min the batch's smallest (1.0f exactly at beta == 0). With S == 0 the
 * batch has no window (m = 0 throughout). One workgroup per learner; deterministic. */
int mz_drqn_prio_sample(uint64_t seed, uint64_t counter, int32_t hidden, int32_t E, int32_t L,
                        int32_t T, int32_t K, int64_t capacity, const int32_t* mem_len_dev,
                        const uint32_t* mem_prio_dev, const uint64_t* mem_psum_dev,
                        int32_t* wdir_dev, int64_t* win_off_dev, int64_t* win_tot_dev,
                        float* isw_dev, double beta, void* stream);

/* After the source net's mz_drqn_window_forward and before mz_drqn_window_backward. For window e
 * over its m training rows: a_i = |qa_i - y_i| (f32), pr = eta max a_i + (1 - eta) mean a_i
 * (float64, the mean summed in time order, both products and the sum rounded separately), mass =
 * clamp(llrint(pow(pr + eps, alpha) 2^20), 1, 2^30) (2^30 where that is not finite; alpha == 0
 * gives 2^20 exactly), written to mem_prio_dev[slot][(b + k) / T]; prio_max_dev[0] becomes the
 * maximum of itself and the batch's masses (an integer atomic). Once all E are written, every
 * touched slot's mem_psum_dev is recomputed from its W entries. Then d_dev[row] *= isw_dev[e] for
 * the window's training rows and ep_loss_dev[e] *= (double) isw_dev[e], so the unchanged backward
 * gives the gradient and value of sum_e w_e sum_t (Q_t[a_t] - y_t)^2 / sum m. One workgroup per
 * learner; a window the directory does not describe validly is skipped. */
int mz_drqn_prio_update(int32_t hidden, int32_t E, int32_t L, int32_t T, int64_t capacity,
                        const int32_t* wdir_dev, const int64_t* win_off_dev,
                        const int64_t* win_tot_dev, const float* qa_dev, const float* y_dev,
                        float* d_dev, double* ep_loss_dev, const float* isw_dev, double alpha,
                        double eta, double eps, uint32_t* mem_prio_dev, uint64_t* mem_psum_dev,
                        uint32_t* prio_max_dev, void* stream);

/* ---- Populations of recurrent DQN learners (VectorRecurrentDQNPopulation) ---------------------
 * P independent learners of agents/lstm_dqn_agent.py (nn.LSTMCell(6, 32) + nn.Linear(32, 4),
 * whole episodes from SequentialExperienceReplayMemory, lib/replay_memory.py:26-43) advanced by
 * the same launches over B = P b instances; learner p owns instances [p b, (p + 1) b). Each is,
 * bit for bit, what the single-learner entry points above compute on its block: the same device
 * code runs on learner p's rows. params_dev (and the gradient, the AdamW moments) is ONE device
 * buffer, flat [P][5252] f32, a row in state_dict order (weight_ih, weight_hh, bias_ih, bias_hh,
 * fc.weight, fc.bias). Per-learner scalars are device arrays of P; due_dev (int32 [P], NULL: all)
 * marks the learners an update touches: nothing of a learner with due_dev[p] == 0 is written.
 * Every entry point refuses a null pointer, P < 1, b < 1, E < 1, hidden != 32 and capacity < E
 * with MZ_EINVAL before any GPU call. */

/* mz_drqn_act for every learner: instance i of learner p acts from row p of params_dev with
 * eps_dev[p], its Philox draw keyed by (seed_dev[p], counter, i - p b). A workgroup stages one
 * learner's parameters, so the grid is P x ceil(b / 16). h_dev / c_dev stay [32][P b]; t_dev,
 * the records, act_out_dev and q_out_dev are indexed by the global instance as in mz_drqn_act,
 * with the same rules for t_dev and L == 0. */
int mz_drqn_pop_act(const float* params_dev, int32_t hidden, int32_t P, int32_t b,
                    const float* obs6_dev, int32_t L, const float* eps_dev,
                    int32_t explore_actions, const uint64_t* seed_dev, uint64_t counter,
                    const int32_t* t_dev, float* h_dev, float* c_dev, float* rec_x_dev,
                    int32_t* rec_a_dev, int32_t* act_out_dev, float* q_out_dev, void* stream);

/* mz_drqn_store for every learner, after mz_ppo_scan over all P b instances: the finished list
 * is in instance order, so learner p's episodes are a contiguous run of it, and the k-th of that
 * run goes into slot (head_p + k) mod capacity of learner p's ring (the last `capacity` of a
 * longer run stay). mem_dev [P][capacity][L + 1][8] words, mem_len_dev / mem_term_dev
 * [P][capacity], ring_dev int64 [P][2]. A learner with no finished episode has nothing written. */
int mz_drqn_pop_store(const float* obs6_dev, const uint8_t* term_dev, int32_t P, int32_t b,
                      int32_t L, const int32_t* fin_id_dev, const int32_t* fin_len_dev,
                      const int32_t* fin_count_dev, float* rec_x_dev, const int32_t* rec_a_dev,
                      const double* rec_r_dev, int64_t capacity, uint32_t* mem_dev,
                      int32_t* mem_len_dev, int32_t* mem_term_dev, int64_t* ring_dev,
                      void* stream);

/* mz_drqn_sample per due learner, one wave each, keyed by (seed_dev[p], counter_dev[p]) over
 * learner p's filled slots; the directories are [P][E] (dir_tot [P][2]). min_filled is the
 * caller's knowledge of the smallest ring count among the due learners; E > min_filled is
 * refused. */
int mz_drqn_pop_sample(const uint64_t* seed_dev, const uint64_t* counter_dev,
                       const int32_t* due_dev, int32_t P, int32_t E, int32_t L, int64_t capacity,
                       int64_t min_filled, const int64_t* ring_dev, const int32_t* mem_len_dev,
                       int32_t* dir_slot_dev, int32_t* dir_len_dev, int64_t* dir_off_dev,
                       int64_t* dir_tot_dev, void* stream);

/* mz_drqn_seq_forward per due learner: one wave per (learner, episode). The row buffers are
 * [P][E (L + 1)] (stash_dev [P][E (L + 1)][192], ep_loss_dev [P][E]); dir_off counts rows within
 * the learner's own buffer. gamma_dev: f32 [P] (source mode; may be NULL with target != 0). */
int mz_drqn_pop_seq_forward(const float* params_dev, int32_t hidden, int32_t target, int32_t P,
                            int32_t E, int32_t L, int64_t capacity, const float* gamma_dev,
                            const int32_t* due_dev, const uint32_t* mem_dev,
                            const int32_t* mem_term_dev, const int32_t* dir_slot_dev,
                            const int32_t* dir_len_dev, const int64_t* dir_off_dev,
                            const int64_t* dir_tot_dev, float* qmax_dev, float* stash_dev,
                            float* qa_dev, float* y_dev, float* d_dev, double* ep_loss_dev,
                            void* stream);

/* mz_drqn_seq_backward per due learner: gpart_dev [P][E][5252]; each learner's E partials are
 * summed in episode order (float64, rounded once) into row p of grads_dev (flat [P][5252],
 * overwritten) and loss_dev[p]. No atomics. */
int mz_drqn_pop_seq_backward(const float* params_dev, int32_t hidden, int32_t P, int32_t E,
                             int32_t L, int64_t capacity, const int32_t* due_dev,
                             const uint32_t* mem_dev, const int32_t* dir_slot_dev,
                             const int32_t* dir_len_dev, const int64_t* dir_off_dev,
                             const int64_t* dir_tot_dev, const float* stash_dev,
                             const float* d_dev, const double* ep_loss_dev, float* gpart_dev,
                             float* grads_dev, float* loss_dev, void* stream);

/* ---- Replay windows in a population ------------------------------------------------------------
 * Learner p is mz_drqn_window_* on its rows with (T, K_p, stored or zero state), bit for bit. T is
 * shared by the population and fixes the layouts; burn_in_dev (int32 [P]) holds the K_p, K_max is
 * their largest, stored_dev (int32 [P]) says which learners read the state memory. mz_drqn_snapshot
 * is called as it is with B = P b. Every entry point refuses a null pointer, P < 1, b < 1, E < 1,
 * T < 1, K_max < 0, K_max % T != 0, hidden != 32, L < 1 and capacity < E with MZ_EINVAL before any
 * GPU call, as far as it has the argument. A burn_in_dev[p] that is negative, not a multiple of T or
 * above K_max cannot be refused by the host, which never reads the array: the caller validates the
 * values before it uploads them. On the device such a learner gets no window (its directory has
 * b = k = m = 0 and win_tot 0), none of its row buffers is written, its partials, its gradient row
 * and its loss are zero, and every access stays within the buffers. */

/* mz_drqn_snap_store for every learner, BEFORE mz_drqn_pop_store of the same vector step (whose
 * ring launch advances the heads read here): learner p's run of the finished list by
 * mz_drqn_pop_store's rule and validity tests, the snapshots of its k-th episode into slot
 * (head_p + k) mod capacity of mem_state_dev [P][capacity][ceil(L / T)][64]. snap_rec_dev is
 * [P b][ceil(L / T)][64], indexed by the global instance. A learner with no finished episode has
 * nothing written; snapshot 0 and the entries past an episode's windows are never written. */
int mz_drqn_pop_snap_store(int32_t hidden, int32_t P, int32_t b, int32_t L, int32_t T,
                           const int32_t* fin_id_dev, const int32_t* fin_len_dev,
                           const int32_t* fin_count_dev, const float* snap_rec_dev,
                           int64_t capacity, float* mem_state_dev, const int64_t* ring_dev,
                           void* stream);

/* mz_drqn_window_sample per due learner, one wave each, keyed by (seed_dev[p], counter_dev[p])
 * with K = burn_in_dev[p]. wdir_dev is int32 [P][5][E], one single-learner directory per learner;
 * win_off_dev [P][E] counts rows within the learner's own buffers; win_tot_dev [P][2]. min_filled
 * as in mz_drqn_pop_sample. */
int mz_drqn_pop_window_sample(const uint64_t* seed_dev, const uint64_t* counter_dev,
                              const int32_t* burn_in_dev, const int32_t* due_dev, int32_t hidden,
                              int32_t P, int32_t E, int32_t L, int32_t T, int32_t K_max,
                              int64_t capacity, int64_t min_filled, const int64_t* ring_dev,
                              const int32_t* mem_len_dev, int32_t* wdir_dev, int64_t* win_off_dev,
                              int64_t* win_tot_dev, void* stream);

/* mz_drqn_window_forward per due learner: one wave per (learner, window). Learner p starts from
 * mem_state_dev's snapshots where stored_dev[p] != 0 and from zero state otherwise; a NULL
 * mem_state_dev is zero state for all (stored_dev may then be NULL). The row buffers are
 * [P][E (min(T, L) + 2)] (stash_dev [...][192]), ep_loss_dev [P][E]. gamma_dev: f32 [P] (source
 * mode; may be NULL with target != 0). */
int mz_drqn_pop_window_forward(const float* params_dev, int32_t hidden, int32_t target, int32_t P,
                               int32_t E, int32_t L, int32_t T, int32_t K_max, int64_t capacity,
                               const float* gamma_dev, const int32_t* burn_in_dev,
                               const int32_t* stored_dev, const int32_t* due_dev,
                               const uint32_t* mem_dev, const int32_t* mem_term_dev,
                               const float* mem_state_dev, const int32_t* wdir_dev,
                               const int64_t* win_off_dev, const int64_t* win_tot_dev,
                               float* qmax_dev, float* stash_dev, float* qa_dev, float* y_dev,
                               float* d_dev, double* ep_loss_dev, void* stream);

/* mz_drqn_window_backward per due learner: gpart_dev [P][E][5252]; each learner's E partials are
 * summed in window order (float64, rounded once) into row p of grads_dev (flat [P][5252],
 * overwritten) and loss_dev[p] = its sum of ep_loss / sum m. No atomics. */
int mz_drqn_pop_window_backward(const float* params_dev, int32_t hidden, int32_t P, int32_t E,
                                int32_t L, int32_t T, int32_t K_max, int64_t capacity,
                                const int32_t* burn_in_dev, const int32_t* due_dev,
                                const uint32_t* mem_dev, const int32_t* wdir_dev,
                                const int64_t* win_off_dev, const int64_t* win_tot_dev,
                                const float* stash_dev, const float* d_dev,
                                const double* ep_loss_dev, float* gpart_dev, float* grads_dev,
                                float* loss_dev, void* stream);

/* ---- Double-Q targets and n-step returns (double_q=..., n_step=...) -------------------------------
 * The update's chain when a learner leaves the defaults (population entry points only; the single
 * trainer is P = 1): the target net's forward and the source net's in the forms below, then the
 * returns kernel, which forms y, d and ep_loss; mz_drqn_pop_prio_update and the backwards follow as
 * they are. The old forwards are not part of the chain and keep their bits. Two more row buffers:
 * q4_dev f32 [P][rows][4], the target net's four Q' of a row (16-byte aligned), and sel_dev int32
 * [P][rows], the first argmax of the source net's own Q (the acting kernel's rule: the first maximum
 * in action order, 0 for a NaN row); rows as the old forwards' row buffers. With a span of training
 * steps s .. s + m - 1 in rows row .. row + m - 1 (a whole episode: s = 0, m = n; a window: after
 * its burn-in), both cover rows row .. row + m: row + m is the step after the last training step,
 * the guard row of a window, row off + n of an episode.
 *
 * The forwards take the old forwards' arguments without gamma_dev and mem_term_dev, which only y
 * read, and with q4_dev / sel_dev in place of qmax_dev / y_dev / d_dev / ep_loss_dev. target != 0:
 * the target net writes q4_dev for rows row .. row + m (stash_dev, qa_dev, sel_dev may be NULL).
 * target == 0: the source net unrolls one step further than the old forward, x_{s+m} from its own
 * state; it writes the stash and qa_dev for the training rows as the old forward does (the same
 * bits) and sel_dev for rows row .. row + m; the extra step has no stash row, no loss term and no
 * gradient (q4_dev may be NULL). Refusals as the old forwards'. */
int mz_drqn_pop_seq_forward_q(const float* params_dev, int32_t hidden, int32_t target, int32_t P,
                              int32_t E, int32_t L, int64_t capacity, const int32_t* due_dev,
                              const uint32_t* mem_dev, const int32_t* dir_slot_dev,
                              const int32_t* dir_len_dev, const int64_t* dir_off_dev,
                              const int64_t* dir_tot_dev, float* q4_dev, float* stash_dev,
                              float* qa_dev, int32_t* sel_dev, void* stream);
int mz_drqn_pop_window_forward_q(const float* params_dev, int32_t hidden, int32_t target, int32_t P,
                                 int32_t E, int32_t L, int32_t T, int32_t K_max, int64_t capacity,
                                 const int32_t* burn_in_dev, const int32_t* stored_dev,
                                 const int32_t* due_dev, const uint32_t* mem_dev,
                                 const float* mem_state_dev, const int32_t* wdir_dev,
                                 const int64_t* win_off_dev, const int64_t* win_tot_dev,
                                 float* q4_dev, float* stash_dev, float* qa_dev, int32_t* sel_dev,
                                 void* stream);

/* After both forwards, one wave per (learner, span), with N = n_step_dev[p] (int32 [P]) and
 * gamma_dev[p]. For training step t of the span: k = min(N, s + m - t), u = t + k (the return is cut
 * at the span's end: no reward past it is read), boot = q4[u][sel[u]] where learner p is double,
 * else max_a q4[u][a]; no bootstrap where u == n and the episode terminated. In float32, in this
 * order: acc = no_boot ? r_{u-1} : fmaf(gamma, boot, r_{u-1}); acc = fmaf(gamma, acc, r_i) for
 * i = u - 2 down to t; y_t = acc; d_t = 2 (qa_t - y_t) (float)(1.0 / tot[1]); ep_loss_dev[p][e] =
 * the float64 sum of the squared residuals in time order. N = 1 without sel_dev gives the old source
 * forward's y, d and ep_loss bit for bit. sel_dev NULL: every learner bootstraps from the max;
 * otherwise learner p reads it where double_dev[p] != 0 (int32 [P]; NULL: every learner does). No
 * atomics; rows outside the directory's spans are not touched. Refused: null pointers (but
 * sel_dev, double_dev, due_dev), the old forwards' sizes, n_step_max < 1. n_step_dev lives on the
 * device and cannot be refused: a value outside 1 .. n_step_max counts as the nearer bound. */
int mz_drqn_pop_seq_returns(const int32_t* n_step_dev, int32_t n_step_max,
                            const int32_t* double_dev, const float* gamma_dev,
                            const int32_t* due_dev, int32_t P, int32_t E, int32_t L,
                            int64_t capacity, const uint32_t* mem_dev, const int32_t* mem_term_dev,
                            const int32_t* dir_slot_dev, const int32_t* dir_len_dev,
                            const int64_t* dir_off_dev, const int64_t* dir_tot_dev,
                            const float* qa_dev, const float* q4_dev, const int32_t* sel_dev,
                            float* y_dev, float* d_dev, double* ep_loss_dev, void* stream);
int mz_drqn_pop_window_returns(const int32_t* n_step_dev, int32_t n_step_max,
                               const int32_t* double_dev, const float* gamma_dev,
                               const int32_t* burn_in_dev, const int32_t* due_dev, int32_t P,
                               int32_t E, int32_t L, int32_t T, int32_t K_max, int64_t capacity,
                               const uint32_t* mem_dev, const int32_t* mem_term_dev,
                               const int32_t* wdir_dev, const int64_t* win_off_dev,
                               const int64_t* win_tot_dev, const float* qa_dev,
                               const float* q4_dev, const int32_t* sel_dev, float* y_dev,
                               float* d_dev, double* ep_loss_dev, void* stream);

/* ---- Prioritized replay windows per learner (VectorRecurrentDQNPopulation(priority_alpha=...)) --
 * The three mz_drqn_prio_* kernels over P learners in one launch each, learner p on its own rows:
 * mem_prio_dev uint32 [P][capacity][W], mem_psum_dev uint64 [P][capacity], prio_max_dev uint32 [P],
 * isw_dev f32 [P][E]; the directory, win_off_dev, win_tot_dev and the row buffers as the
 * mz_drqn_pop_window_* entry points lay them out. Learner p's outputs are, bit for bit, what the
 * single entry point writes on its block with its values. due_dev (int32 [P], may be NULL: all
 * due): a learner with due_dev[p] == 0 has nothing read or written. Each refuses, before any GPU
 * call, P < 1, b < 1, any other null pointer, and all the single entry points refuse. The
 * per-learner values (beta_dev, alpha_dev, eta_dev, eps_dev, burn_in_dev) live on the device and
 * cannot be refused here: the caller validates them before it uploads them. */

/* mz_drqn_prio_store for every learner, BEFORE mz_drqn_pop_store of the same vector step: learner
 * p's run of the finished list by mz_drqn_pop_store's rule, its k-th episode's windows into slot
 * (head_p + k) mod capacity at the mass prio_max_dev[p]. ring_dev is int64 [P][2]. */
int mz_drqn_pop_prio_store(int32_t hidden, int32_t P, int32_t b, int32_t L, int32_t T,
                           const int32_t* fin_id_dev, const int32_t* fin_len_dev,
                           const int32_t* fin_count_dev, int64_t capacity, uint32_t* mem_prio_dev,
                           uint64_t* mem_psum_dev, const uint32_t* prio_max_dev,
                           const int64_t* ring_dev, void* stream);

/* mz_drqn_prio_sample per due learner, one workgroup each, keyed by (seed_dev[p], counter_dev[p])
 * with K = burn_in_dev[p] (<= K_max) and the importance exponent beta_dev[p] (float64 [P], each
 * finite and >= 0). T is shared. */
int mz_drqn_pop_prio_sample(const uint64_t* seed_dev, const uint64_t* counter_dev,
                            const int32_t* burn_in_dev, const double* beta_dev,
                            const int32_t* due_dev, int32_t hidden, int32_t P, int32_t E, int32_t L,
                            int32_t T, int32_t K_max, int64_t capacity, const int32_t* mem_len_dev,
                            const uint32_t* mem_prio_dev, const uint64_t* mem_psum_dev,
                            int32_t* wdir_dev, int64_t* win_off_dev, int64_t* win_tot_dev,
                            float* isw_dev, void* stream);

/* mz_drqn_prio_update per due learner, one workgroup each, with alpha_dev[p] (finite, >= 0),
 * eta_dev[p] (in [0, 1]) and eps_dev[p] (finite, > 0), float64 [P] each: between
 * mz_drqn_pop_window_forward (source) and mz_drqn_pop_window_backward. */
int mz_drqn_pop_prio_update(const double* alpha_dev, const double* eta_dev, const double* eps_dev,
                            const int32_t* due_dev, int32_t hidden, int32_t P, int32_t E, int32_t L,
                            int32_t T, int64_t capacity, const int32_t* wdir_dev,
                            const int64_t* win_off_dev, const int64_t* win_tot_dev,
                            const float* qa_dev, const float* y_dev, float* d_dev,
                            double* ep_loss_dev, const float* isw_dev, uint32_t* mem_prio_dev,
                            uint64_t* mem_psum_dev, uint32_t* prio_max_dev, void* stream);

/* The target sync (lstm_dqn_agent.py update_target: target.load_state_dict(source.state_dict()))
 * of the learners with mask_dev[p] != 0: row p of dst_dev <- row p of src_dev ([P][5252]). */
int mz_drqn_pop_sync(const float* src_dev, float* dst_dev, const int32_t* mask_dev, int32_t P,
                     void* stream);

/* mz_adamw_flat's clamp + AdamW (dqn_agent.py:152-157) over rows [P][n] (n a multiple of 4, the
 * buffers 16-byte aligned): row p at lr_dev[p] with step count step_dev[p] (f32, advanced by
 * one), the element arithmetic shared with mz_adamw_flat, so one row gives the same bits. A row
 * with due_dev[p] == 0 keeps its parameters, moments, gradient and step count. */
int mz_adamw_pop(float* param_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* grad_dev,
                 int32_t P, int64_t n, const float* lr_dev, float* step_dev,
                 const int32_t* due_dev, double beta1, double beta2, double eps,
                 double weight_decay, float clamp, float grad_scale, int32_t write_grad,
                 void* stream);

/* ---- The DQN / DDQN acting forward, f32-accurate on the bf16 MFMA (mz_qact.hip) -------------
 * Replaces, per acting row, source_net(state).max(1)[1] (dqn_agent.py:113-116; the nets of
 * dqn_agent.py:19-57 / ddqn_agent.py:18-52 at the reference's sizes: Conv2d(3, 32, 3, p 1),
 * 1,574 -> 1,024 -> 512 -> 4). Every GEMM operand is split into bf16 hi + lo and each product
 * summed as hi*hi + hi*lo + lo*hi in f32 (~2^-16 relative): the f32 argmax at bf16-MFMA speed. */

/* fc1's weight [1024][1574] (torch layout) and fc2's [512][1024] f32 -> the hi / lo bf16 images
 * mz_qact reads, in MFMA fragment order (a wave's operand for one K chunk contiguous): w1 1024 x 1600
 * elements (features in the kernel's order, zero pad), w2 512 x 1024. Every pointer 16-B aligned (MZ_EINVAL otherwise). */
int mz_qact_prepare(const float* fc1_w_dev, const float* fc2_w_dev, uint16_t* w1_hi_dev,
                    uint16_t* w1_lo_dev, uint16_t* w2_hi_dev, uint16_t* w2_lo_dev, void* stream);

/* Q values and greedy actions of min(n, *count_dev) rows (count_dev NULL: n): row i is instance
 * rows_dev[i] (rows_dev NULL: instance i) of bits_dev [B][22] / obs6_dev [B][6]. Conv weight
 * [32][3][3][3] / bias, fc1 bias [1024], fc2 bias [512], fc3 weight [4][512] / bias [4] f32;
 * relu: 1 for DDQN's second activation (ReLU), 0 for DQN's LeakyReLU; drop_p > 0: DDQN's
 * train-mode Dropout after the conv activation (counter hash of seed / counter, row, feature).
 * h1_dev: workspace of mz_qact_workspace_floats(n) f32 (fc1's output rows [n][1024], then the
 * conv stem's bf16 hi / lo feature tiles: the stem runs once per 64 rows, k_qconv, and fc1 reads
 * them, k_qfc1). Outputs: greedy_dev[instance] = first argmax (int64; NaN as torch.argmax),
 * q_out_dev [n][4] f32 (either may be NULL). No host synchronisation. */
int64_t mz_qact_workspace_floats(int32_t n);
int mz_qact(const uint32_t* bits_dev, const float* obs6_dev, const int32_t* rows_dev,
            const int32_t* count_dev, int32_t n, const float* conv_w_dev, const float* conv_b_dev,
            const uint16_t* w1_hi_dev, const uint16_t* w1_lo_dev, const float* b1_dev,
            const uint16_t* w2_hi_dev, const uint16_t* w2_lo_dev, const float* b2_dev,
            const float* w3_dev, const float* b3_dev, int32_t relu, float drop_p, uint64_t seed,
            uint64_t counter, float* h1_dev, int64_t* greedy_dev, float* q_out_dev, void* stream);

/* ---- Config 1 vectorised: a population of tabular Q-learners in HBM (mz_qtab.hip) ------------
 * Replaces, per instance, QAgent (agents/q_agent.py:8-79: a dict of 4-entry float64 rows keyed
 * by str(obs)) and the step / episode end of OffPolicyTrainer.train (lib/trainers/
 * off_policy_trainer.py:28-80). n instances, one lane each, on the PLAIN observation obs6_dev
 * [n][6] = (r, c, gr, gc, br, bc) as exact small integers in f32 (an enrich = 0 handle's obs6;
 * 8-B aligned). Instance i learns on table table_of_dev[i] (NULL: table i, ntables == n) of
 * q_dev [ntables][rows][4] float64 (16-B aligned, zero = the reference's fresh rows). Every
 * hyper-parameter and counter is a per-table device array [ntables]. Entries of table_of_dev
 * outside [0, ntables) make the instance idle (action -1, no update).
 *
 * Index layout: row = (((r * P + c) * P + gr) * P + gc) * 5 + k with P = max_dim, rows = 5 P^4
 * (mz_qtab_states), k the best-dir class: 0 (0, 0); 1 down: br == -1 or br > 1; 2 up: br == 1 or
 * br < -1; 3 right: bc == -1 or bc > 1; 4 left: bc == 1 or bc < -1 (|x| > 1 is the torus'
 * wrapped neighbour, +-(N - 1)). Two observations of one env share a row iff their str(obs) keys
 * are equal. Coordinates are clamped to [0, P), so no access leaves a table. */

/* rows per table for pitch max_dim (5 <= max_dim <= MZ_MAX_DIM). */
int mz_qtab_states(int32_t max_dim, int64_t* rows);

/* QAgent.get_action (q_agent.py:44-54) for every instance: eps = final + (init - final) *
 * exp(-1.0 * steps_done[t] / decay) in float64; draws mz_philox(seed, MZ_QTAB_STREAM ^ (i << 32),
 * counter): u = (w0 >> 8) * 2^-24; u < eps -> action w1 >> 30 (action_space.sample(), uniform
 * over 4; not mz_act's masked distribution), else the row's first maximum (np.argmax). Writes
 * actions_dev (int32 [n], mz_step's input) and sidx_dev (int64 [n], the row acted from), then
 * steps_done_dev[t] += the instances acting on t (never reset, like QAgent's). Instances with
 * active_dev[i] == 0 (uint8 [n], NULL: all act) idle: action -1, row -1, not counted (an
 * evaluation's instances whose episode is over). Two launches. */
int mz_qtab_act(const float* obs6_dev, int32_t n, int32_t max_dim, const int32_t* table_of_dev,
                int32_t ntables, const uint8_t* active_dev, const double* q_dev,
                int64_t* steps_done_dev, const double* eps_init_dev, const double* eps_final_dev,
                const double* eps_decay_dev, uint64_t seed, uint64_t counter, int32_t* actions_dev,
                int64_t* sidx_dev, void* stream);

/* QAgent.update (q_agent.py:56-73) after mz_step, obs6_dev now the next observation, in float64
 * in this order: future = terminated ? 0 : max(Q[s']); td = (reward + gamma * future) - Q[s][a];
 * Q[s][a] = Q[s][a] + lr * td. Then cum_dev[i] += reward and, on terminated | truncated,
 * gamma[t] += cum > 0 ? eta : -eta (update_hyperparameter(cumulative > prev_cum_rew) with
 * prev_cum_rew zeroed every episode, off_policy_trainer.py:32,77-78), cum = 0, episodes[t] += 1,
 * wins[t] += terminated. episode_end == 0: QAgent.update alone — cum still sums, but no gamma
 * drift and no counters (a caller that ends episodes itself, or never calls
 * update_hyperparameter).
 * table_of_dev NULL: one launch, plain stores. Otherwise (shared tables) two launches: every td
 * of the step is computed from the table and gamma as they stood before the step (lr * td into
 * td_dev, n float64, required), then applied with one native float64 global atomic add per
 * instance — colliding updates add; gamma and the counters take atomic adds too. Disjoint rows
 * give the bits of the one-launch form; colliding adds arrive in no fixed order, so their sum is
 * bitwise reproducible only when the addends commute exactly. */
int mz_qtab_update(const float* obs6_dev, int32_t n, int32_t max_dim, const int32_t* table_of_dev,
                   int32_t ntables, double* q_dev, const int64_t* sidx_dev,
                   const int32_t* actions_dev, const double* reward64_dev,
                   const uint8_t* terminated_dev, const uint8_t* truncated_dev, double* gamma_dev,
                   const double* lr_dev, const double* eta_dev, double* cum_dev,
                   int64_t* episodes_dev, int64_t* wins_dev, double* td_dev, int32_t episode_end,
                   void* stream);

/* ---- The same learner on hashed tables (mz_qtab.hip) ------------------------------------------
 * QAgent's table is a defaultdict(lambda: np.zeros(4)) (agents/q_agent.py:8-79) that holds only
 * the states met; a dense table holds all 5 P^4 (452 MB at 41x41, 6.9 GB at 81x81). Here each of
 * the ntables tables is an open-addressing hash table of `capacity` slots (a power of two,
 * 16 <= capacity <= 2^30, the same for all tables):
 *   keys_dev     int32 [ntables][capacity]     key = the dense row index above (< 5 * 127^4 <
 *                                              2^31 for every legal pitch); -1 = empty
 *   vals_dev     f64   [ntables][capacity][4]  32-B aligned, zero-filled by the caller: an absent
 *                                              key reads as the zero row (np.zeros(4))
 *   load_dev     int32 [ntables]               occupied slots
 *   overflow_dev int64 [ntables]               updates dropped because the table was full
 * Hash: slot0 = (uint32(key) * 0x9E3779B1u) >> (32 - log2 capacity), then +1 mod capacity. Every
 * probe ends after at most `capacity` slots. Table full: a lookup answers absent; an update's
 * value is dropped and overflow_dev[t] += 1, its episode-end bookkeeping (cum, gamma +- eta,
 * episodes, wins) still runs; no error. Keys are never deleted. Lookups and concurrent inserts
 * never share a launch. Argument errors (capacity not such a power of two, null pointers, a
 * negative count) are refused before any GPU call. */

/* mz_qtab_act with the row fetched by lookup (QAgent.get_action, q_agent.py:44-54): read-only on
 * the tables — acting never inserts. sidx_dev receives the dense key acted from. Two launches. */
int mz_qtab_hash_act(const float* obs6_dev, int32_t n, int32_t max_dim,
                     const int32_t* table_of_dev, int32_t ntables, const uint8_t* active_dev,
                     const int32_t* keys_dev, const double* vals_dev, int64_t capacity,
                     int64_t* steps_done_dev, const double* eps_init_dev,
                     const double* eps_final_dev, const double* eps_decay_dev, uint64_t seed,
                     uint64_t counter, int32_t* actions_dev, int64_t* sidx_dev, void* stream);

/* mz_qtab_update on hashed tables (QAgent.update, q_agent.py:56-73, and the episode end of
 * off_policy_trainer.py:32,77-78), the same float64 operations in the same order. table_of_dev
 * NULL: one launch — look up s' and s, td, find or insert s, store Q[s][a] + lr * td (the key is
 * inserted on every write, also of a zero value; load_dev[t] += 1 on a new slot). Otherwise two
 * launches: the read-only td pass (td_dev required), then find-or-insert — a slot is claimed by
 * a 32-bit compare-and-swap of its key from -1; a lane that loses uses the slot if it now holds
 * its own key and probes on otherwise — and one float64 atomic add on the value. */
int mz_qtab_hash_update(const float* obs6_dev, int32_t n, int32_t max_dim,
                        const int32_t* table_of_dev, int32_t ntables, int32_t* keys_dev,
                        double* vals_dev, int64_t capacity, int32_t* load_dev,
                        int64_t* overflow_dev, const int64_t* sidx_dev, const int32_t* actions_dev,
                        const double* reward64_dev, const uint8_t* terminated_dev,
                        const uint8_t* truncated_dev, double* gamma_dev, const double* lr_dev,
                        const double* eta_dev, double* cum_dev, int64_t* episodes_dev,
                        int64_t* wins_dev, double* td_dev, int32_t episode_end, void* stream);

/* Re-insert every (key, row) of the ntables tables into new_keys_dev / new_vals_dev of capacity
 * new_capacity, which the caller has filled with -1 / zero and which must not overlap the old
 * arrays. One lane per old slot, the same compare-and-swap claim. The load counters carry over
 * unchanged; an entry that finds its new table full is dropped and counted in overflow_dev (size
 * new_capacity above the largest load and none is). */
int mz_qtab_hash_rehash(const int32_t* keys_dev, const double* vals_dev, int64_t capacity,
                        int32_t* new_keys_dev, double* new_vals_dev, int64_t new_capacity,
                        int32_t ntables, int64_t* overflow_dev, void* stream);

/* For m (table, key) pairs — tables_dev int32 [m], query_keys_dev int64 [m] — rows_out_dev
 * [m][4] float64 (16-B aligned; zeros if absent) and slots_out_dev int32 [m] (-1 if absent, also
 * for a table outside [0, ntables) or a key outside [0, 2^31)). m == 0 does nothing. */
int mz_qtab_hash_lookup(const int32_t* keys_dev, const double* vals_dev, int64_t capacity,
                        int32_t ntables, const int32_t* tables_dev,
                        const int64_t* query_keys_dev, int32_t m, double* rows_out_dev,
                        int32_t* slots_out_dev, void* stream);

/* ---- Double Q-learning populations (mz_qtab.hip) ----------------------------------------------
 * Replaces, per instance, DQAgent (agents/dq_agent.py:5-73: two dicts of 4-entry float64 rows,
 * q_a_values and q_b_values, keyed by str(obs)) under the same OffPolicyTrainer.train. Everything
 * above holds (the index, the per-table arrays, idle instances, the hash and its probe) except
 * the row: a state's A row and B row sit side by side, [2][4] float64 = 64 B, 64-B aligned.
 *   dense    q_dev    [ntables][rows][2][4]
 *   hashed   keys_dev int32 [ntables][capacity] as above (one key per state, one probe for both
 *            tables), vals_dev [ntables][capacity][2][4]; a write to either table inserts the key.
 * Argument errors (null pointers, a negative count, a bad pitch, a capacity that is not a power
 * of two in [16, 2^30], a misaligned table) are refused before any GPU call. */

/* DQAgent.get_action (dq_agent.py:35-46): mz_qtab_act on the A row — acting reads Q_A only; the
 * same MZ_QTAB_STREAM draw, the same steps_done advance. Two launches. */
int mz_dqtab_act(const float* obs6_dev, int32_t n, int32_t max_dim, const int32_t* table_of_dev,
                 int32_t ntables, const uint8_t* active_dev, const double* q_dev,
                 int64_t* steps_done_dev, const double* eps_init_dev, const double* eps_final_dev,
                 const double* eps_decay_dev, uint64_t seed, uint64_t counter, int32_t* actions_dev,
                 int64_t* sidx_dev, void* stream);

/* DQAgent.update (dq_agent.py:48-66) after mz_step, then mz_qtab_update's episode end
 * (dq_agent.py:69-73 is QAgent's update_hyperparameter). Draws mz_philox(seed, MZ_DQTAB_STREAM ^
 * (i << 32), ucounter), ucounter the caller's count of update calls:
 *   (w0 >> 8) * 2^-24 < 0.5 -> table A is updated, else B (:57);
 *   best = get_action(next_obs) (:58, :62), the inner eps-greedy choice on Q_A[s'] in either case:
 *   eps from steps_done_dev[t] as this call finds it (after the act's advance), u2 = (w1 >> 8) *
 *   2^-24 < eps -> best = w2 >> 30, else the first maximum of Q_A[s'];
 *   updating A: td = (reward + gamma * Q_B[s'][best]) - Q_A[s][a]; Q_A[s][a] = Q_A[s][a] + lr * td
 *   (:59-60), updating B: the same with A and B swapped (:63-64). No terminated factor, as there.
 * took_dev (uint8 [n], required) receives 1 where a td was computed; a last launch adds these
 * inner get_actions to steps_done_dev (steps_done grows by 2 per training step), after every
 * lane read the old value.
 * coin_dev (uint8 [n]; 0 = A, 1 = B; NULL: draw) and next_action_dev (int32 [n] in 0..3, outside:
 * the instance idles; NULL: the inner choice) replace the draws, for replaying the reference; with
 * next_action_dev no eps is evaluated, steps_done still advances.
 * table_of_dev NULL: two launches. Otherwise three: a read-only pass writes lr * td into td_dev
 * (float64 [n]) and the chosen table into which_dev (uint8 [n]), both required then; a second
 * does one float64 atomic add per instance into the chosen table's element, and the episode end
 * with atomic adds. */
int mz_dqtab_update(const float* obs6_dev, int32_t n, int32_t max_dim, const int32_t* table_of_dev,
                    int32_t ntables, double* q_dev, const int64_t* sidx_dev,
                    const int32_t* actions_dev, const double* reward64_dev,
                    const uint8_t* terminated_dev, const uint8_t* truncated_dev, double* gamma_dev,
                    const double* lr_dev, const double* eta_dev, double* cum_dev,
                    int64_t* episodes_dev, int64_t* wins_dev, double* td_dev, int32_t episode_end,
                    int64_t* steps_done_dev, const double* eps_init_dev,
                    const double* eps_final_dev, const double* eps_decay_dev, uint64_t seed,
                    uint64_t ucounter, const uint8_t* coin_dev, const int32_t* next_action_dev,
                    uint8_t* took_dev, uint8_t* which_dev, void* stream);

/* mz_dqtab_act on hashed tables (dq_agent.py:35-46): the A row by lookup, absent -> zeros; acting
 * never inserts. Two launches. */
int mz_dqtab_hash_act(const float* obs6_dev, int32_t n, int32_t max_dim,
                      const int32_t* table_of_dev, int32_t ntables, const uint8_t* active_dev,
                      const int32_t* keys_dev, const double* vals_dev, int64_t capacity,
                      int64_t* steps_done_dev, const double* eps_init_dev,
                      const double* eps_final_dev, const double* eps_decay_dev, uint64_t seed,
                      uint64_t counter, int32_t* actions_dev, int64_t* sidx_dev, void* stream);

/* mz_dqtab_update on hashed tables (dq_agent.py:48-66): look up s' and s, the same draws and td,
 * find or insert s (shared tables: the compare-and-swap claim of mz_qtab_hash_update, in the
 * second pass), store or add into the chosen table's element. A full table drops the write and
 * counts overflow_dev[t]; the dropped update still counts its get_action and its episode end. */
int mz_dqtab_hash_update(const float* obs6_dev, int32_t n, int32_t max_dim,
                         const int32_t* table_of_dev, int32_t ntables, int32_t* keys_dev,
                         double* vals_dev, int64_t capacity, int32_t* load_dev,
                         int64_t* overflow_dev, const int64_t* sidx_dev,
                         const int32_t* actions_dev, const double* reward64_dev,
                         const uint8_t* terminated_dev, const uint8_t* truncated_dev,
                         double* gamma_dev, const double* lr_dev, const double* eta_dev,
                         double* cum_dev, int64_t* episodes_dev, int64_t* wins_dev, double* td_dev,
                         int32_t episode_end, int64_t* steps_done_dev, const double* eps_init_dev,
                         const double* eps_final_dev, const double* eps_decay_dev, uint64_t seed,
                         uint64_t ucounter, const uint8_t* coin_dev,
                         const int32_t* next_action_dev, uint8_t* took_dev, uint8_t* which_dev,
                         void* stream);

/* mz_qtab_hash_rehash for the 64-B slots of DQAgent's two dicts (dq_agent.py:17-18). */
int mz_dqtab_hash_rehash(const int32_t* keys_dev, const double* vals_dev, int64_t capacity,
                         int32_t* new_keys_dev, double* new_vals_dev, int64_t new_capacity,
                         int32_t ntables, int64_t* overflow_dev, void* stream);

/* mz_qtab_hash_lookup for the 64-B slots (dq_agent.py:17-18): rows_out_dev [m][2][4] float64, the
 * A row then the B row (16-B aligned; zeros if absent). */
int mz_dqtab_hash_lookup(const int32_t* keys_dev, const double* vals_dev, int64_t capacity,
                         int32_t ntables, const int32_t* tables_dev,
                         const int64_t* query_keys_dev, int32_t m, double* rows_out_dev,
                         int32_t* slots_out_dev, void* stream);

/* ---- Explored-maze archive (mz_archive.hip) --------------------------------------------------
 * Replaces `env.mazes`, the list the reference env appends every maze it trains on to (the first
 * one and each update_maze() replacement: simple_maze_env.py:34,91,
 * simple_variable_maze_env.py:39,106), and update_visited_maze(), which puts one back for
 * test(n, new=False) (off_policy_trainer.py:84-119). The CALLER owns all archive memory (device
 * arrays); the handle keeps no pointer to it, so an archive outlives its handle, can be saved and
 * can be loaded into another handle.
 *
 * One entry = one maze of size N <= P (P = the archive's pitch, a handle's max_dim):
 *   bits  int32 [W], W = ceil(P * P / 32) (mz_archive_words): bit (r * N + c) & 31 of word
 *         (r * N + c) >> 5 is 1 iff cell (r, c) is open (grid value 1 or 2) — row-major with the
 *         entry's own N; the bits at index >= N * N and all remaining words are 0;
 *   meta  int32 [2]: the instance's meta words, N | N << 8 | start_r << 16 | start_c << 24 and
 *         goal_r | goal_c << 8 | max_steps << 16 (toroidal handles: the cropped coordinates, as
 *         held);
 *   algo  uint8: the instance's algorithm id. */

/* W for pitch max_dim (5 <= max_dim <= MZ_MAX_DIM). Runs on the host (as mz_qtab_states). */
int mz_archive_words(int32_t max_dim, int32_t* words);

/* env.mazes.append(maze) (simple_maze_env.py:34,91) for every instance e with flags_dev[e] != 0
 * (NULL: all): its current maze goes to slot count_dev[e] % slots of its ring — bits_dev
 * [B][slots][words], meta_dev [B][slots][2], algo_dev [B][slots] — then count_dev[e] += 1 (count_dev
 * [B], non-negative). One writer per instance, no atomics; the handle's state is only read.
 * words must equal mz_archive_words(the handle's max_dim) and slots >= 1 (else MZ_EINVAL). One
 * launch, asynchronous. */
int mz_archive_push(mz_handle* h, const uint8_t* flags_dev, int32_t slots, int32_t words,
                    int32_t* bits_dev, int32_t* meta_dev, uint8_t* algo_dev, int32_t* count_dev,
                    void* stream);

/* update_visited_maze() (off_policy_trainer.py:96-116) without the host: target j = instance
 * env_ids_dev[j] (NULL: j; the listed ids must differ) becomes the maze of linear entry
 * slot_dev[j] of bits_dev [entries][words], meta_dev [entries][2], algo_dev [entries] — the caller
 * keeps 0 <= slot_dev[j] < entries; a negative slot leaves the instance alone. Built as
 * mz_load_mazes builds an imported maze, bit for bit (distance field, cell words, plane strips,
 * max_steps, meta, the instance reset, its last-terminated flag cleared), with the entry's
 * algorithm id, and with targets of different sizes in one launch. One launch, asynchronous, no
 * host copy. Every entry is validated on the device before anything is stored: N odd,
 * 5 <= N <= the handle's max_dim (>= 15 on an euclidean enrich handle), N * N bits inside `words`
 * (the SOURCE arrays' row length: an archive of another pitch is legal as long as N fits), start
 * and goal inside N with both bits set, algorithm id 0..2, instance id inside the handle. A bad
 * entry leaves its instance untouched and adds 1 to *errors_dev (int32, zeroed by the caller). */
int mz_archive_load(mz_handle* h, const int32_t* env_ids_dev, int32_t n, const int32_t* slot_dev,
                    int32_t words, const int32_t* bits_dev, const int32_t* meta_dev,
                    const uint8_t* algo_dev, int32_t* errors_dev, void* stream);

/* The explored-maze pool: ONE list for the whole population, `env.mazes` of a learner that trains
 * on B envs at once, filled in exploration order — by call, and within a call by instance id.
 * It keeps the first `capacity` entries and counts the rest. An entry is the archive entry above
 * plus owner (the instance id) and stamp (the caller's, e.g. the vector step). Read one back with
 * mz_archive_load: its slots are the entry numbers.
 *
 * mz_archive_pool_span: the instances one workgroup of the push covers (a multiple of 64; host
 * only) — the sizes at which a test crosses workgroups. */
int mz_archive_pool_span(int32_t* span);

/* Let c = *count_dev before the call and F = the instances with flags_dev[i] != 0 in ascending id
 * (NULL: all). The r-th instance of F becomes entry c + r of bits_dev [capacity][words], meta_dev
 * [capacity][2], algo_dev / owner_dev / stamp_dev [capacity] if c + r < capacity, otherwise it is
 * dropped; nothing at or past `capacity` is written. The new count is min(c + |F|, INT32_MAX):
 * held = min(count, capacity), dropped = max(count - capacity, 0).
 * THE COUNT IS A TWO-WORD COUNTER: count_dev (4-byte aligned) points at the word that holds c,
 * one of an 8-byte-aligned pair of int32. The call only reads it and writes the new count to the
 * OTHER word of the pair, (uintptr_t)count_dev ^ 4; the caller passes that other word to its
 * next call. No workgroup then reads a word another one writes: the result does not depend on the
 * order in which workgroups run, and calls issued back to back on one stream behave as sequential
 * calls. One launch, asynchronous, no host read. The handle's state is only read.
 * MZ_EINVAL before any launch: a null handle or array, capacity < 1, words != mz_archive_words(
 * the handle's max_dim), a misaligned count_dev. */
int mz_archive_push_pool(mz_handle* h, const uint8_t* flags_dev, int32_t capacity, int32_t words,
                         int32_t* bits_dev, int32_t* meta_dev, uint8_t* algo_dev,
                         int32_t* owner_dev, int32_t* stamp_dev, int32_t* count_dev, int32_t stamp,
                         void* stream);

/* One pool per learner of a population of learners: the handle's B instances are `groups` groups
 * of b = B / groups consecutive instances, and group g has a pool of its own — rows
 * [g * capacity, (g + 1) * capacity) of bits_dev [groups * capacity][words], meta_dev
 * [groups * capacity][2], algo_dev / owner_dev / stamp_dev [groups * capacity] — and a two-word
 * counter of its own, count_dev [groups][2] (8-byte aligned). One launch appends the flagged
 * instances of every group g (flags_dev [B], NULL: all) to pool g in ascending instance id, from
 * entry count_dev[g][parity] on, exactly as mz_archive_push_pool would on a handle that held
 * group g's b instances alone: owner is the instance's id within its group, i - g * b; nothing is
 * written at or past entry `capacity` of a pool; count_dev[g][parity ^ 1] becomes
 * min(count + flagged in group g, INT32_MAX) and count_dev[g][parity] is only read. The caller
 * passes parity ^ 1 to its next call. groups == 1 is mz_archive_push_pool, bit for bit. No
 * atomics and nothing exchanged between workgroups: every slot is a function of the flags alone.
 * One launch, asynchronous, no host read. The handle's state is only read.
 * MZ_EINVAL before any launch: a null handle or array, groups < 1, B % groups != 0,
 * capacity < 1, words != mz_archive_words(the handle's max_dim), a count_dev that is not 8-byte
 * aligned, a parity other than 0 or 1. */
int mz_archive_push_pools(mz_handle* h, const uint8_t* flags_dev, int32_t groups, int32_t capacity,
                          int32_t words, int32_t* bits_dev, int32_t* meta_dev, uint8_t* algo_dev,
                          int32_t* owner_dev, int32_t* stamp_dev, int32_t* count_dev,
                          int32_t parity, int32_t stamp, void* stream);

#ifdef __cplusplus
}
#endif
#endif
