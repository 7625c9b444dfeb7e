/*
 * libtd3hip -- C ABI of the MI355X-native TD3 gradient step (gfx950).
 *
 * Plain pointers and sizes only; no torch types.  Every function returns 0 on
 * success, -1 on an argument error and -2 on a HIP / RCCL error; the message of
 * the last failure on the calling thread is td3_last_error().
 *
 * Each entry point replaces one piece of the reference's Python surface
 * (/root/reference, duck-typed classes selected at main.py:203-208):
 *
 *   rb_create            ReplayBuffer_featured.__init__   my_replay_buffer.py:73-89
 *   rb_add               ReplayBuffer_featured.add        my_replay_buffer.py:109-117
 *   rb_sample            ReplayBuffer_featured.sample     my_replay_buffer.py:119-128
 *   rb_read/write_records ReplayBuffer_featured.save/load my_replay_buffer.py:91-107
 *   rb_*_particles       ReplayBuffer_particles          my_replay_buffer.py:6-69
 *   td3_create           TD3.__init__ + TD3_base.__init__ TD3_featured.py:100-110, TD3_base.py:7-24
 *   td3_get/set_params   state_dict()/load_state_dict()   TD3_base.py:26-50 (save/load)
 *   td3_train_step       TD3.train(replay_buffer, B)      TD3_featured.py:123-171
 *   td3_train_step_batch TD3.train on a foreign buffer's sample() tensors
 *   td3_select_action    TD3.select_action                TD3_featured.py:113-115
 *   td3_eval_q           TD3.eval_q                       TD3_featured.py:117-121
 *   rb_add_device        ReplayBuffer_featured.add on device rows (GPU-resident environments)
 *   td3_select_action_device  select_action + OU noise + clip on device rows  main.py:249-252, utils/noise.py
 *   td3_eval_q_device    TD3.eval_q on device rows
 *   td3_*_particles      TD3_particles.TD3 (set encoder)  TD3_particles.py:136-224
 *   rb_add_particles_device   ReplayBuffer_particles.add on device rows  my_replay_buffer.py:46-56
 *   rb_add_device_hindsight / rb_add_particles_device_hindsight
 *                        add_to_replay_buffer with --hindsight_number K on device rows: each
 *                        transition and its K relabels in one fan-out add      main.py:70-91
 *   rb_add_device_nstep / rb_add_particles_device_nstep
 *                        n-step returns on device rows (no counterpart in the reference): each tick's
 *                        rows are stored and the previous n-1 ticks' rows mature in the ring, in one launch
 *   rb_enable_priorities / rb_set_priorities / rb_update_priorities / rb_sample_prioritized /
 *   td3_train_step_prioritized / td3_train_step_prioritized_particles
 *                        prioritized experience replay on the device ring (no counterpart in the
 *                        reference): a 64-ary sum tree next to the ring, the weighted critic loss
 *                        of either learner
 *   rs_create / rs_tick / rs_get_state / rs_set_state / rs_read_episodes / rs_info
 *                        rollout statistics of a GPU-resident vector environment (no counterpart in the
 *                        reference): running observation / reward normalisation and the episode log,
 *                        one launch per tick
 *   rb_state_moments / rb_normalize_states / rb_norm_info
 *                        dataset normalisation (TD3+BC's state normalisation; no counterpart in the reference):
 *                        a loaded ring's state moments into an rs handle and the ring normalised in place
 *   td3_log_enable / td3_log_info / td3_log_read / td3_log_set
 *                        the training log (no counterpart in the reference): per-step losses and Q
 *                        statistics of either learner in a device ring, one opt-in launch per logged step
 *   td3_set_bc / td3_bc_info
 *                        TD3+BC (Fujimoto & Gu 2021; no counterpart in the reference): the behaviour-cloning
 *                        term of the featured actor step, for buffers the learner did not collect
 *                        (experience_injection.py, main.py --load_replay_buffer)
 *   td3_train_step_mixed
 *                        demonstration replay (DDPGfD / RLPD symmetric sampling; the online half of
 *                        experience_injection.py + main.py --load_replay_buffer): every batch draws a fixed
 *                        number of rows from a demonstration ring and the rest from the online ring
 *   td3_set_bc_filter / td3_bc_filter_info / td3_bc_filter_keep
 *                        the BC term on the demonstration rows of a mixed batch only, with a Q-filter (Nair et
 *                        al. 2018; no counterpart in the reference): fine-tuning on top of demonstrations
 *   td3_set_grad_clip / td3_clip_info
 *                        torch.nn.utils.clip_grad_norm_ between backward() and step() (one line with the
 *                        reference's torch classes): global-norm clipping of either group's gradient, on device
 *   td3_select_action_particles_device / td3_eval_q_particles_device
 *                        the particle learner's select_action (+ noise + clip) / eval_q on device rows
 *   td3_actor_learn_particles TD3_particles.TD3._actor_learn TD3_particles.py:209-224
 *   td3_comm_init(_local) data-parallel extension (the reference is single-device)
 *
 * Ownership: handles own all device memory.  Host pointers are owned by the caller
 * and only read/written during the call.  Device pointers passed in (rb_sample
 * outputs, td3_train_step_batch inputs) must stay valid until the stream work of
 * the call has completed.
 *
 * Streams: `stream` arguments are hipStream_t passed as void*; NULL selects the
 * handle's own stream.  td3_train_step orders itself after the ring's last
 * rb_add / rb_fill_synthetic (a transition added at step t is samplable at t,
 * main.py:261 before :269), and a later write after the steps that read the ring.
 * The ordering is recorded lazily (replay.h Ring::read_stream): accesses on one
 * stream need no events, an access on another stream records one on the stream
 * the ring last noted.  A caller stream passed to these calls must therefore stay
 * alive until the ring's next access on another stream, or until rb_destroy;
 * td3_destroy releases the handle's own streams from every ring.  Handles are not
 * re-entrant.
 */
#ifndef TD3_HIP_H
#define TD3_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rb_handle rb_handle;
typedef struct td3_handle td3_handle;

/* ------------------------------------------------------------------ replay ring */
typedef struct rb_info_t {
  int state_dim, action_dim;
  int record_floats;       /* floats per HBM record: [s | a | s2 | r | not_done | pad] */
  int64_t max_size, ptr, size;
  void* data;              /* device pointer of the ring [max_size][record_floats] */
  int device;
  int n_particles, particle_dim;   /* particle rings (state_dim = feature dim); 0 otherwise */
} rb_info_t;

int rb_create(int state_dim, int action_dim, int64_t max_size, int device, uint64_t seed,
              rb_handle** out);
int rb_destroy(rb_handle* h);
int rb_info(const rb_handle* h, rb_info_t* info);
/* The ring's own stream (hipStream_t): the stream a NULL `stream` argument selects.  Callers
 * that consume rb_sample outputs on another stream order it after this one. */
void* rb_stream(rb_handle* h);
/* n transitions, row-major float64 host arrays (reference dtype); stores 1-done. */
int rb_add(rb_handle* h, const double* state, const double* action, const double* next_state,
           const double* reward, const double* done, int64_t n, void* stream);
/* n packed float32 records (record_floats each). */
int rb_add_records(rb_handle* h, const float* records, int64_t n, void* stream);
/* n transitions from DEVICE float32 arrays (contiguous: state [n][sd], action [n][ad],
 * next_state [n][sd], reward [n], done [n]) into ring rows ptr, ptr+1, ... (wrapping);
 * stores not_done = 1.0f - done, zeroes the record pad.  n > max_size keeps the last max_size rows
 * (as rb_add).  Asynchronous on `stream` (NULL: the ring's own); inputs must stay valid until that
 * stream's work has completed.  The records are assembled in the ring by one kernel: no staging
 * buffer, no host copy.  Featured rings only: a particle ring returns -1 (rb_add_particles_device). */
int rb_add_device(rb_handle* h, const float* state, const float* action, const float* next_state,
                  const float* reward, const float* done, int64_t n, void* stream);
/* Device-side synthetic prefill (SURVEY.md §8d distribution), n rows at ptr. */
int rb_fill_synthetic(rb_handle* h, int64_t n, float max_action, uint64_t seed, void* stream);
/* Gather `batch` rows into device outputs state[B][sd], action[B][ad], next_state[B][sd],
 * reward[B], not_done[B].  inject_idx (device, nullable) replaces the Philox draw;
 * idx_out (device, nullable) receives the rows drawn. */
int rb_sample(rb_handle* h, int batch, float* state, float* action, float* next_state,
              float* reward, float* not_done, const int64_t* inject_idx, int64_t* idx_out,
              void* stream);
int rb_read_records(const rb_handle* h, int64_t start, int64_t n, float* out);
int rb_write_records(rb_handle* h, int64_t start, int64_t n, const float* in, int64_t ptr,
                     int64_t size);
int rb_sync(rb_handle* h);

/* TD3_particles ring (ReplayBuffer_particles, my_replay_buffer.py:6-69).  Record:
 * [feat(F) | particles(N*D) | action(A) | next_feat(F) | next_particles(N*D) | r | not_done | pad]. */
int rb_create_particles(int feat_dim, int n_particles, int particle_dim, int action_dim, int64_t max_size,
                        int device, uint64_t seed, rb_handle** out);
/* float64 host rows: feat [n][F], part [n][N][D], action [n][A], ... (my_replay_buffer.py:46-56) */
int rb_add_particles(rb_handle* h, const double* feat, const double* part, const double* action,
                     const double* next_feat, const double* next_part, const double* reward,
                     const double* done, int64_t n, void* stream);
/* rb_add_particles from DEVICE float32 arrays (contiguous: feat / next_feat [n][F], part / next_part
 * [n][N*D], action [n][A], reward [n], done [n]): the records [feat | particles | action | next_feat |
 * next_particles | r | not_done | pad] are assembled in ring rows ptr, ptr+1, ... (wrapping) by one
 * kernel, with not_done = 1.0f - done and a zeroed pad; ptr / size and n > max_size as rb_add_device.
 * The source rows need no alignment (N*D may be odd): every source float is read once, the ring is
 * written with aligned 16-byte stores.  Asynchronous on `stream` (NULL: the ring's own), no staging
 * buffer, no host copy; inputs must stay valid until that stream's work has completed.  A featured
 * ring returns -1 (rb_add_device). */
int rb_add_particles_device(rb_handle* h, const float* feat, const float* part, const float* action,
                            const float* next_feat, const float* next_part, const float* reward,
                            const float* done, int64_t n, void* stream);
/* Hindsight fan-out adds (main.py:70-91 on device rows): each of the n source transitions is stored
 * 1 + k times.  With E[i*(1+k)] = transition i unchanged and E[i*(1+k) + j] (j = 1..k) = the same
 * transition with goals[i][j-1][0..g) written into feature columns cols[0..g) of BOTH state and
 * next_state (feat and next_feat on a particle ring) and rewards[i][j-1] as its reward, the ring
 * records, ptr and size after the call are bit for bit those of rb_add_device /
 * rb_add_particles_device given the n*(1+k) rows of E: rows ptr, ptr+1, ... (wrapping), only the last
 * max_size rows of E when n*(1+k) > max_size (the first surviving row may be a relabel in the
 * middle of a transition), not_done = 1.0f - done, a zeroed pad.  The source rows are read once per
 * transition by the particle form (the two particle blocks are not re-read per copy).
 * Asynchronous on `stream` and ordered exactly as the plain device adds; the device inputs, goals and
 * rewards included, must stay valid until that stream's work has completed, `hs` itself is host
 * memory read during the call only.  Checked in this order, each failure returning -1 with a message
 * naming the field: n >= 0; hs (non-null, k, g, goals, rewards, cols non-negative and distinct);
 * the handle; the ring kind (as rb_add_device / rb_add_particles_device); cols below state_dim
 * (particle rings: feat_dim).  n == 0 then returns 0. */
typedef struct rb_hindsight {
  int k;                 /* relabels per transition, 1..64 */
  int g;                 /* goal columns, 1..8 */
  int cols[8];           /* distinct feature columns in [0, state_dim) (particle rings: [0, feat_dim)) */
  const float* goals;    /* device [n][k][g] */
  const float* rewards;  /* device [n][k] */
} rb_hindsight;
int rb_add_device_hindsight(rb_handle* h, const float* state, const float* action, const float* next_state,
                            const float* reward, const float* done, int64_t n, const rb_hindsight* hs,
                            void* stream);
int rb_add_particles_device_hindsight(rb_handle* h, const float* feat, const float* part, const float* action,
                                      const float* next_feat, const float* next_part, const float* reward,
                                      const float* done, int64_t n, const rb_hindsight* hs, void* stream);
/* N-step adds: rb_add_device / rb_add_particles_device for a vectorised rollout whose stored rows
 * mature in the ring into multi-step transitions.  One call is one tick: `rows` environments, source
 * row i always the same environment.  The tick's rows go to ring rows ptr, ptr+1, ... (wrapping) exactly
 * as the plain device add stores them (not_done = 1.0f - done, a zeroed pad), and the same launch
 * updates, for every environment whose episode is still running, the rows its previous up to n-1
 * ticks stored: the row of j ticks ago gets reward += gpow[j] * reward[i] (fp32), this tick's
 * next_state (particle rings: next_feat and next_particles) and not_done = gpow[j] * (1.0f - done[i]);
 * its state, action (and feat / particles) columns keep their bits.  gpow[j] = (float) of the double
 * product of j factors gamma, multiplied left to right; gpow[0] = 1.  A row stops maturing with the
 * tick at which its environment has `ended` or done != 0, or after n ticks.
 * Closed form: over the ticks 0..T-1 of one uninterrupted lane, with e the first tick >= t at which
 * environment i has ended or done set (or infinity) and m = min(n, e - t + 1, T - t), the row of
 * environment i's transition (s_t, a_t, r_t, s'_t, d_t) holds s_t, a_t, s'_{t+m-1},
 * reward = sum_{k<m} gamma^k r_{t+k} and not_done = gpow[m-1] * (1 - d_{t+m-1}): at every moment an
 * exact m-step transition for the learners' target y = r + (not_done * discount) * min Q', 1 <= m <= n,
 * with no flush at episode ends and a fixed row count per tick.  The caller is responsible for gamma
 * equalling the learner's discount.  rb_sample* and save() return the not_done column as stored, so it
 * may be fractional.  n = 1 stores exactly what the plain device add stores.
 * A lane is the run of consecutive n-step calls with the same rows, n and gamma; a call with another
 * of these, and every other call that writes the ring (rb_add, rb_add_records, rb_add_device, both
 * hindsight adds, the particle adds, rb_fill_synthetic, rb_write_records), ends it: the earlier rows stay
 * as they are (a valid shorter horizon) and the next n-step call starts a fresh lane.
 * Asynchronous on `stream`, ordered and with the pointer lifetimes of rb_add_device (`ended` included);
 * `ns` itself is host memory read during the call only.  Checked in this order, each failure returning
 * -1 with a message naming the field, before any GPU work and leaving ring, lane, ptr and size unchanged:
 * rows >= 0; ns (non-null, n, gamma, ended); the handle; the ring kind (as rb_add_device /
 * rb_add_particles_device); n * rows <= max_size (unlike the plain add, a tick is never truncated).
 * rows == 0 then returns 0 and leaves the lane alone. */
typedef struct rb_nstep {
  int n;                  /* horizon, 1..8; 1 stores exactly what the plain device add stores */
  double gamma;           /* the learner's discount, in (0, 1] */
  const uint8_t* ended;   /* device [rows]: nonzero -> this row's episode ended with this transition,
                             time limits included; a row with done != 0 counts as ended too */
} rb_nstep;
int rb_add_device_nstep(rb_handle* h, const float* state, const float* action, const float* next_state,
                        const float* reward, const float* done, int64_t rows, const rb_nstep* ns, void* stream);
int rb_add_particles_device_nstep(rb_handle* h, const float* feat, const float* part, const float* action,
                                  const float* next_feat, const float* next_part, const float* reward,
                                  const float* done, int64_t rows, const rb_nstep* ns, void* stream);
/* The 7 tensors of ReplayBuffer_particles.sample (:58-69) into device outputs. */
int rb_sample_particles(rb_handle* h, int batch, float* feat, float* part, float* action, float* next_feat,
                        float* next_part, float* reward, float* not_done, const int64_t* inject_idx,
                        int64_t* idx_out, void* stream);

/* Prioritized replay (Schaul et al. 2016): optional per-row priorities of a ring of either kind, kept
 * outside the records in a 64-ary sum tree (level 0: one fp32 leaf per row; each higher level one fp32
 * per 64 nodes below, every level zero-padded to a multiple of 64, up to a single root group of 64;
 * max_size = 10^6 gives 4 levels).  rb_info_t, the record layout, rb_read_records / rb_write_records and
 * save() files do not change, and a ring without priorities queues not one extra launch or byte.
 * At every stream-ordered point between calls: a leaf is > 0 exactly for the rows < size that hold a
 * transition (unless rb_set_priorities stored a 0); every inner node is the sum of its 64 children as
 * last recomputed; max_priority (a device scalar, 1.0f at first) is at least every priority stored so
 * far; the total mass is the sum of the root group.  Sums are never updated by deltas or float atomics:
 * a store writes the leaves and then, level by level, recomputes every affected parent from all 64 of
 * its children in one fixed order, so duplicate indices are harmless and the tree is bit for bit
 * reproducible.
 * New rows: every call that writes the ring gives the rows it wrote max_priority, on the stream of the
 * write -- rb_add, rb_add_records, rb_add_device, rb_add_particles(_device), both hindsight adds (all
 * n*(1+k) rows), both n-step adds (the tick's new rows only: rows that mature in place keep their
 * priority), rb_fill_synthetic; rb_write_records gives rows [0, size) max_priority and the rest 0.
 * rb_enable_priorities: allocates the tree and gives rows [0, size) priority 1.0f, on `stream`, ordered
 *   as a ring write.  Checked in this order: alpha in [0, 1]; eps > 0; the handle; not already enabled.
 * rb_set_priorities: leaves idx[i] = p[i] as given (DEVICE arrays; finite and >= 0; neither alpha nor
 *   eps is applied; 0 takes the row out of the draw), raises max_priority, repairs the parents.  A
 *   row named several times in one call ends with the largest of its values, whatever the order.
 * rb_update_priorities: the same with p = powf(td_abs[i] + eps, alpha) in fp32 (a non-finite result
 *   stores the current max_priority instead).  Both are asynchronous on `stream`, ordered as a ring
 *   write, and check in this order: n >= 0; non-null idx and values when n > 0; the handle; priorities
 *   enabled.  n == 0 returns 0.  Indices are trusted to be < max_size, as rb_sample's inject_idx is.
 * rb_sample_prioritized: `batch` rows drawn in proportion to their priorities into idx_out, their
 *   importance weights into weight_out (DEVICE arrays [batch]); asynchronous on `stream`, ordered as a
 *   ring read.  The draw is stratified: draw k has the mass fraction u_k = (k + U_k) / batch (fp32,
 *   kept below 1), U_k in [0, 1) from Philox4x32-10 with the ring's seed as key and the counter
 *   (k, stream id 5, step lo, step hi) -- a stream id of its own next to the learner's target noise (2)
 *   and the exploration draw (4) -- where step is the ring's sample-call counter (shared with rb_sample,
 *   advanced by every call); with inject_u (device [batch], nullable) u_k = inject_u[k] itself.  The mass
 *   m = u_k * total is one fp32 multiply.  Descent, from the root group down: the first child whose
 *   inclusive prefix sum (fp32, in the order the parents were summed) exceeds m, m less the prefix
 *   before it; where rounding leaves none, the last child with a non-zero value.  A row of priority 0 is
 *   never returned.  weight_out[k] = w_k / max_j w_j with w = (size * p / total)^(-beta) in fp32: the
 *   weights are normalised by the maximum of the BATCH (as Dopamine does), not of the buffer, which
 *   would need a min-tree for no practical gain.  Checked in this order: batch > 0; beta in [0, 1];
 *   non-null outputs; the handle; priorities enabled; size > 0.
 * rb_get_priorities: leaves [start, start + n) to the host; synchronous.
 * rb_priority_info: synchronous; a ring without priorities reports enabled = 0 (and returns 0: this is
 *   the query for it); every other call above returns -1 on such a ring.
 * Every failure returns -1 before any GPU work, with a message naming the field. */
typedef struct rb_priority_info_t {
  int enabled;
  double alpha, eps;
  int levels;
  double total;            /* the root sum, widened from the device's fp32 */
  float max_priority;
} rb_priority_info_t;
int rb_enable_priorities(rb_handle* h, double alpha, double eps, void* stream);
int rb_set_priorities(rb_handle* h, const int64_t* idx, const float* p, int64_t n, void* stream);
int rb_update_priorities(rb_handle* h, const int64_t* idx, const float* td_abs, int64_t n, void* stream);
int rb_sample_prioritized(rb_handle* h, int batch, double beta, const float* inject_u, int64_t* idx_out,
                          float* weight_out, void* stream);
int rb_get_priorities(const rb_handle* h, int64_t start, int64_t n, float* host_out);
int rb_priority_info(const rb_handle* h, rb_priority_info_t* info);

/* ------------------------------------------------------------------ rollout statistics */
/* Per-tick bookkeeping of a GPU-resident vector environment (no counterpart in the reference; what gym's
 * NormalizeObservation / NormalizeReward wrappers and main.py:240-289's episode prints do on the host):
 * running observation moments and normalisation, running moments of the discounted return and reward
 * scaling, and a log of finished episodes -- none of it read back per tick.  An rs_handle owns, for `rows`
 * environments of `obs_dim` columns, all in device memory:
 *   observation moments  count, mean[obs_dim], m2[obs_dim]                       (fp64)
 *   return moments       ret_count, ret_mean, ret_m2, the accumulator G[rows]    (fp64)
 *   episode accounting   ep_return[rows] (fp64), ep_len[rows] (int32)
 *   episode log          a ring of log_cap rs_episode entries; ep_count, ep_len_sum, tick (int64),
 *                        ep_return_sum (fp64)
 * It touches neither a learner nor a replay ring: the rows a caller stores are simply the normalised ones.
 * fp64 throughout: a running mean over 10^8 rows of columns spanning orders of magnitude loses what fp32
 * carries, fp64 vector arithmetic is cheap on this part, and the data of a tick is a few hundred KB.
 *
 * rs_tick is one call per environment tick and EXACTLY ONE KERNEL LAUNCH (rs_tick_kernel; none when no
 * input is given): asynchronous on `stream`, no host read-back, no allocation.  Unlike the ring and
 * learner calls a NULL `stream` is HIP's default (null) stream itself -- the handle owns no stream; torch's
 * default stream is that one, so a tick queued there is ordered with the torch ops around it.
 * Device inputs (each nullable): obs [rows][obs_dim], the rows the next actions are chosen from (after
 * auto-reset); next_obs [rows][obs_dim], the transition's own next state; reward [rows]; ended [rows]
 * (nonzero: the row's episode ended with this transition).  Device outputs (each nullable, each may alias
 * its own input and nothing else): obs_out, next_obs_out, reward_out.  In this order:
 *  1. Observation moments, only with update = 1 and obs given.  Per enabled column: the batch sum, then
 *     mb = sum / rows, then m2b = sum (x - mb)^2, in fp64 and in an order fixed by (rows, obs_dim): column
 *     c is summed by P = 1024 / W row phases, phase p over rows p, p + P, ... in row order, the phases
 *     combined by a halving tree (p += p + s, s = P/2, ..., 1); W is the largest power of two <= 64 with
 *     rows * W <= 8192 (at least 1), halved while W / 2 >= obs_dim, and a workgroup owns W columns.
 *     Chan's merge: d = mb - mean, tot = count + rows, mean += d * rows / tot,
 *     m2 += m2b + d * d * count * rows / tot, count = tot.  No float atomics: runs repeat bit for bit.
 *  2. Normalise obs and next_obs where given with an output, both with the moments as they stand after 1:
 *     an enabled column gets out = (float) clip((x - mean) / sqrt(m2 / count + obs_eps), +-obs_clip),
 *     evaluated in fp64 and rounded to fp32 once; with count == 0 and in a masked column out = x bit for bit.
 *  3. Reward, only with reward given.  G_i = gamma * G_i + r_i.  With update = 1 the batch moments of G over
 *     the rows (row i in partial i mod 1024, the partials by the same halving tree) are merged into the
 *     return moments by the same formula.  reward_out_i = (float) clip(r_i / sqrt(ret_m2 / ret_count +
 *     rew_eps), +-rew_clip) in fp64 (r_i itself while ret_count == 0).  Then G_i = 0 where ended_i.
 *  4. Episodes, whenever reward is given, whatever `update`: ep_return_i += r_i (the raw reward),
 *     ep_len_i += 1; for the rows with ended_i IN INCREASING ROW ORDER the entry {(float) ep_return_i,
 *     ep_len_i, i, tick} goes to log slot ep_count mod log_cap, ep_count += 1, ep_return_sum += ep_return_i,
 *     ep_len_sum += ep_len_i, and the row's two accumulators are zeroed.  Then tick += 1 (a call without a
 *     reward, e.g. the one after reset(), is not a tick).
 * update = 0 freezes every moment (evaluation); episodes are still logged.
 * rs_config.col_mask (host uint8 [obs_dim], nullable, read during rs_create only): a zero takes the column
 * out of normalisation -- copied through bit for bit, no moments kept -- e.g. the goal columns a hindsight
 * relabel overwrites with raw goals.
 * rs_get_state / rs_set_state: every moment, accumulator, counter and the whole log ring to / from host
 * arrays of the caller (mean, m2 [obs_dim]; G, ep_return, ep_len [rows]; log [log_cap], slot order);
 * synchronous (they wait for the device), for checkpoints.  rs_read_episodes: the entries with sequence
 * numbers in [first, first + n) that are still in the ring (the last log_cap), oldest first, into out;
 * *first_out is the sequence number of out[0], *n_out the entries written; synchronous.  rs_info: synchronous.
 * A caller's stream must stay alive until its ticks have completed.  Handles are not re-entrant.
 * Checked in this order, each failure returning -1 before any GPU work with a message naming the field:
 *   rs_create: out; rows in 1..2^24; obs_dim in 1..2^20; log_cap in 1..2^24; cfg non-null; cfg->obs_eps
 *     (finite, >= 0); cfg->obs_clip (finite, > 0); cfg->rew_eps; cfg->rew_clip; cfg->gamma in [0, 1].
 *   rs_tick: a non-null; a->update 0 or 1; a->obs_out without a->obs; a->next_obs_out without a->next_obs;
 *     a->reward_out without a->reward; a->ended without a->reward; the handle.
 *   rs_get_state: st non-null; st->mean, m2, G, ep_return, ep_len, log non-null, in this order; the handle.
 *   rs_set_state: the same, then st->count, st->ret_count (finite, >= 0), st->ep_count, st->ep_len_sum,
 *     st->tick (>= 0); the handle.
 *   rs_read_episodes: first >= 0; n >= 0; out non-null unless n == 0; first_out; n_out; the handle.
 *   rs_info: info non-null; the handle.   rs_destroy(NULL) returns 0. */
typedef struct rs_handle rs_handle;
typedef struct rs_config {
  double obs_eps, obs_clip;      /* gym's NormalizeObservation: 1e-8, 10 */
  double rew_eps, rew_clip;      /* gym's NormalizeReward: 1e-8, 10 */
  double gamma;                  /* discount of the return whose spread scales the reward */
  const uint8_t* col_mask;       /* host [obs_dim], nullable: 0 -> the column is passed through */
} rs_config;
typedef struct rs_tick_t {
  const float* obs;              /* device [rows][obs_dim], nullable */
  const float* next_obs;         /* device [rows][obs_dim], nullable */
  const float* reward;           /* device [rows], nullable */
  const uint8_t* ended;          /* device [rows], nullable (needs reward) */
  float* obs_out;                /* device, nullable, may be obs */
  float* next_obs_out;           /* device, nullable, may be next_obs */
  float* reward_out;             /* device, nullable, may be reward */
  int update;                    /* 1: steps 1 and 3 update the moments; 0: frozen */
} rs_tick_t;
typedef struct rs_episode {
  float ret;                     /* the episode's undiscounted return (raw rewards) */
  int32_t len;                   /* its length in ticks */
  int32_t row;                   /* the environment */
  int32_t reserved;              /* 0 */
  int64_t tick;                  /* the tick it ended at */
} rs_episode;
typedef struct rs_info_t {
  int rows, obs_dim, log_cap, device;
  int64_t ep_count, ep_len_sum, tick;
  double ep_return_sum, count, ret_count;
} rs_info_t;
typedef struct rs_state {
  double count;
  double* mean;                  /* host [obs_dim] */
  double* m2;                    /* host [obs_dim] */
  double ret_count, ret_mean, ret_m2;
  double* G;                     /* host [rows] */
  double* ep_return;             /* host [rows] */
  int32_t* ep_len;               /* host [rows] */
  rs_episode* log;               /* host [log_cap], slot order */
  int64_t ep_count, ep_len_sum, tick;
  double ep_return_sum;
} rs_state;
int rs_create(int rows, int obs_dim, int log_cap, int device, const rs_config* cfg, rs_handle** out);
int rs_destroy(rs_handle* h);
int rs_tick(rs_handle* h, const rs_tick_t* a, void* stream);
int rs_info(const rs_handle* h, rs_info_t* info);
int rs_get_state(const rs_handle* h, rs_state* st);
int rs_set_state(rs_handle* h, const rs_state* st);
int rs_read_episodes(const rs_handle* h, int64_t first, int64_t n, rs_episode* out, int64_t* first_out,
                     int64_t* n_out);

/* ------------------------------------------------------------------ dataset normalisation */
/* TD3+BC's second ingredient (Fujimoto & Gu 2021) for a ring that was loaded, not collected: the moments of
 * the ring's states into an rs_handle, and the ring normalised in place with them -- both on the device,
 * nothing read back.  Online rows then come through rs_tick with update = 0 on the same moments and the
 * same element expression, so a row normalised in the ring and a row normalised by a tick have the same bits.
 * (TD3+BC's own code divides by std + 1e-3; here the denominator is sqrt(var + obs_eps), as in rs_tick.)
 *
 * rb_state_moments: the fp64 (count, mean[c], m2[c]) of field 0 of the ring (state; features on a particle
 *   ring) over the valid rows [0, size), for every column rs's col_mask enables, into rs's OBSERVATION
 *   moments.  merge = 0 replaces them (count = size); merge = 1 merges into what is there by rs_tick's own
 *   Chan expressions (d = mb - mean, tot = count + size, mean += d * size / tot,
 *   m2 += m2b + d * d * count * size / tot, count = tot).  Every count copy of rs is set.  The return
 *   moments, the accumulators and the episode log of rs are not touched; a masked column's moments are not
 *   written.  Asynchronous on `stream` (NULL: the ring's own), ordered as a ring READ; rs is the caller's
 *   to order (queue its ticks on the same stream).  Two launches, no float atomics.  The order of every
 *   addition is a function of (size, obs_dim) alone, so runs repeat bit for bit whatever the grid:
 *     - the rows are cut into chunks of R = 1024 consecutive ring rows, chunk k = rows [1024 k, 1024 k + 1024),
 *       and a chunk into micro-blocks of 8 rows (the last of either may be short);
 *     - a micro-block of n rows: s = the sum in row order, mb = s / n, m2b = sum (x - mb)^2 in row order --
 *       never sum x^2 - n mean^2;
 *     - with W the power of two covering min(obs_dim - 256 b, 256) for the column's block b of 256 columns
 *       and P = 256 / W, partial p of a chunk takes the micro-blocks m = p (mod P) in ascending m by Chan's
 *       merge (the first as it is), and the P partials are combined by a halving tree (p takes p + s,
 *       s = P/2, ..., 1);
 *     - second launch: partial l of 64 takes the chunks l, l + 64, ... in ascending order, the 64 by the
 *       same halving tree (l takes l + s, s = 32, ..., 1), then the replace or the merge above.
 * rb_normalize_states: rewrites in place the state and next_state columns (features and next_features) of
 *   the rows [0, size) by rs_tick step 2: out = (float) clip((x - mean) / sqrt(m2 / count + obs_eps),
 *   +-obs_clip) in fp64, rounded once; a masked column, or count == 0, leaves x bit for bit.  Action, reward,
 *   not_done, the pad, the particle blocks and the rows at or past size keep their bits.  One launch,
 *   asynchronous on `stream` (NULL: the ring's own), ordered as a ring WRITE; it ends the n-step lane as every
 *   write does, leaves the priorities alone, and the ring remembers normalized = 1: a second call is refused.
 *   rb_write_records and rb_fill_synthetic clear the flag; adds leave it (they are the caller's normalised rows).
 * rb_norm_info: normalized, the ring's state width, and the rows the normalising call rewrote (0 while
 *   normalized = 0); no GPU work.
 * Checked in this order, each failure returning -1 before any GPU work with a message naming the fault:
 *   rb null; rs null; merge 0 or 1 (rb_state_moments only); rs's obs_dim equals the ring's state width
 *   ("dims"); both on one device; the ring is not empty ("empty"); rb_normalize_states only: the ring is
 *   not "already normalised".   rb_norm_info: info non-null; the handle. */
typedef struct rb_norm_info_t { int normalized; int obs_dim; int64_t rows; } rb_norm_info_t;
int rb_state_moments(rb_handle* rb, rs_handle* rs, int merge, void* stream);
int rb_normalize_states(rb_handle* rb, const rs_handle* rs, void* stream);
int rb_norm_info(const rb_handle* rb, rb_norm_info_t* info);

/* ------------------------------------------------------------------ learner */
/* struct_size:sizeof(td3_config) as the caller compiled it.  td3_default_config sets it and
 * td3_create refuses a config whose struct_size differs from the library's (a binding written
 * against another version of this header), before reading any other field. */
typedef struct td3_config {
  int struct_size;
  int state_dim, action_dim;
  int actor_hidden[3];     /* reference: (500, 400, 300)  TD3_featured.py:19 */
  int critic_hidden[3];    /* reference: (500, 400, 200)  TD3_featured.py:54 */
  int norm;                /* 0: None, 1: "layer" (TD3_featured.py:28-31), 2: "weight_normalization" (:33-35, 68-70; featured only) */
  float max_action;
  double discount, tau, policy_noise, noise_clip;   /* TD3_base.py:9-13 */
  int policy_freq;
  double lr, beta1, beta2, eps;                     /* torch.optim.Adam defaults */
  uint64_t seed;           /* Philox key for index draws and target-policy noise */
  int device;
  int use_graph;           /* 0: direct launches; 1: replay each step variant as a hipGraph;
                              2 (default): graph replay while the GPU has caught up with the host,
                              direct launches while earlier steps are still queued */
  /* TD3_particles (TD3_particles.py): state = (features [F], particles [N][D]); the Q head has
   * action_dim outputs; state_dim = F, hidden widths (500, 400, 300) for actor and critic. */
  int particles;           /* 0: TD3_featured, 1: TD3_particles */
  int n_particles, particle_dim;
  int cdq;                 /* clipped double-Q (CDQ flag, TD3_particles.py:126-133); featured: twin always */
} td3_config;

enum td3_which {
  TD3_ACTOR = 0, TD3_ACTOR_TARGET = 1, TD3_CRITIC = 2, TD3_CRITIC_TARGET = 3,
  TD3_ACTOR_ADAM_M = 4, TD3_ACTOR_ADAM_V = 5, TD3_CRITIC_ADAM_M = 6, TD3_CRITIC_ADAM_V = 7,
  /* gradient arenas (read only): in data-parallel mode the all-reduced SUM of the replicas' batch-mean
   * gradients of the last phase (divide by nranks for the mean); with weight normalization dL/dW.
   * Not written by the single-device fused path (its dW tiles feed Adam directly) -- except for a group
   * that clips its gradient (td3_set_grad_clip): its arena holds the last step's unclipped batch-mean
   * gradient. */
  TD3_ACTOR_GRAD = 8, TD3_CRITIC_GRAD = 9
};

typedef struct td3_step_stats {   /* particles: y / q1 / q2 are [B][action_dim] */
  double critic_loss;      /* mse(Q1,y) + mse(Q2,y)  (TD3_featured.py:148) */
  double actor_loss;       /* -mean Q1(s, pi(s)) on actor steps, else NaN (:159) */
  int actor_step;          /* 1 when the delayed policy update ran (:156) */
  float* y;                /* nullable host [B]: target Q */
  float* q1;               /* nullable host [B] */
  float* q2;               /* nullable host [B] */
  int64_t* idx;            /* nullable host [B]: rows drawn */
  float* noise;            /* nullable host [B][ad]: the N(0,1) draw of randn_like (:132) */
} td3_step_stats;

/* sizeof(td3_config) of this library: a binding checks its own struct against it. */
size_t td3_config_size(void);
/* Reference defaults (TD3_base.py:7-24, TD3_featured.py:100, main.py:112-126).  cfg_size is the
 * caller's sizeof(td3_config): on a mismatch nothing is written and -1 is returned. */
int td3_default_config(td3_config* cfg, size_t cfg_size);
int td3_create(const td3_config* cfg, td3_handle** out);
int td3_destroy(td3_handle* h);

/* Parameter tensors in reference state_dict order (Actor: linears.{0..3}.{weight,bias},
 * lnorms.{0..2}.{weight,bias}; Critic: q1.* then q2.*).  Flat, unpadded. */
int td3_tensor_count(const td3_handle* h, int which_group /*0 actor, 1 critic*/);
int td3_tensor_info(const td3_handle* h, int which_group, int index, char* name, int name_len,
                    int64_t* rows, int64_t* cols);
int64_t td3_num_params(const td3_handle* h, int which_group);
int td3_get_params(td3_handle* h, int which, float* out, int64_t n);
int td3_set_params(td3_handle* h, int which, const float* in, int64_t n);
int td3_get_counters(const td3_handle* h, int64_t* total_it, int64_t* critic_step,
                     int64_t* actor_step);
int td3_set_counters(td3_handle* h, int64_t total_it, int64_t critic_step, int64_t actor_step);
/* Adam hyper-parameters of one optimizer (group 0 actor, 1 critic): torch.optim.Adam's
 * param_groups[0] lr / betas / eps, which Adam.load_state_dict adopts from a checkpoint
 * (TD3_base.py:37-50 loads actor_optimizer / critic_optimizer).  Synchronises the learner. */
int td3_set_adam(td3_handle* h, int group, double lr, double beta1, double beta2, double eps);
int td3_get_adam(const td3_handle* h, int group, double out[4] /* lr, beta1, beta2, eps */);

/* One TD3.train(rb, batch) step.  inject_idx [batch] int64 / inject_noise [batch][ad]
 * float32 are HOST arrays (nullable) replacing the Philox draws (parity testing).
 * stats (nullable) forces a sync and fills losses. */
int td3_train_step(td3_handle* h, rb_handle* rb, int batch, void* stream,
                   const int64_t* inject_idx, const float* inject_noise, td3_step_stats* stats);
/* One TD3.train step on a prioritized draw (featured learners, one device).  On the step's stream,
 * inside one read section of the ring (no add can overwrite a sampled row before its priority is
 * written back): rb_sample_prioritized(batch, beta) straight into the step's index and weight buffers;
 * the gather of those rows; the body of td3_train_step with the critic loss
 * sum_j 1/B sum_r w_r (Q_j,r - y_r)^2, i.e. dL/dQ_j,r = 2/B w_r (Q_j,r - y_r) -- the actor loss is not
 * weighted; rb_update_priorities(rows, td_abs) with td_abs_r = 0.5f * (|Q1_r - y_r| + |Q2_r - y_r|).
 * No host synchronisation unless stats, per, inject_u or inject_noise force one.  inject_u [batch]
 * (host, nullable) replaces the stratified Philox draw as in rb_sample_prioritized, inject_noise as in
 * td3_train_step; stats->idx receives the rows drawn, stats->critic_loss the weighted loss; per
 * (nullable) the weights and td_abs of the step.  Every other step entry point keeps unit weights: the
 * first of them after a prioritized step refills the weight buffer on its own stream before its body.
 * Returns -1 with a message for: a particle learner (its step is td3_train_step_prioritized_particles
 * below); a handle in a td3_comm_init or td3_comm_init_local group; a ring without priorities; a ring
 * whose kind or dims do not match; beta outside [0, 1]; an empty ring. */
typedef struct td3_per_stats {
  float* weight;           /* nullable host [B]: importance weights used */
  float* td_abs;           /* nullable host [B]: the |TD error| written back */
} td3_per_stats;
int td3_train_step_prioritized(td3_handle* h, rb_handle* rb, int batch, double beta, void* stream,
                               const float* inject_u, const float* inject_noise, td3_step_stats* stats,
                               td3_per_stats* per);
/* The same step for a particle learner (TD3_particles) on a prioritized particle ring, one device.
 * With B rows, A = action_dim Q outputs per row, J online critics (2 with CDQ, 1 without) and w_r the
 * importance weight of row r (one per transition, shared by its A outputs): y as td3_train_step;
 * critic loss sum_j 1/(B*A) sum_r w_r sum_o (Q_j,r,o - y_r,o)^2, i.e.
 * dL/dQ_j,r,o = 2/(B*A) w_r (Q_j,r,o - y_r,o) -- the actor loss is not weighted;
 * td_abs_r = 1/(J*A) sum_j sum_o |Q_j,r,o - y_r,o| in float32, each critic's sum over o in increasing
 * order, the critics added in order j (A = 1 with CDQ: the featured step's 0.5f * (|Q1 - y| + |Q2 - y|)).
 * Everything else is td3_train_step_prioritized's contract: one read section of the ring around the
 * draw (into the step's index and weight buffers), the gather of those rows' small fields (the encoders
 * read their particle blocks in the ring), the body and rb_update_priorities(rows, td_abs), where a row
 * drawn twice keeps its larger value; inject_u / inject_noise / stats / per as there
 * (stats->critic_loss the weighted loss, stats->y / q1 / q2 [B][A]); no host synchronisation unless one
 * of those forces it.  Every other particle step entry point (td3_train_step,
 * td3_train_step_batch_particles, td3_actor_learn_particles) keeps unit weights.
 * Returns -1 with a message, before any GPU work, for: a featured learner; a handle in a td3_comm_init
 * or td3_comm_init_local group; a ring without priorities; a ring whose kind or dims do not match; beta
 * outside [0, 1]; an empty ring. */
int td3_train_step_prioritized_particles(td3_handle* h, rb_handle* rb, int batch, double beta, void* stream,
                                         const float* inject_u, const float* inject_noise,
                                         td3_step_stats* stats, td3_per_stats* per);
/* Same step on an already-sampled batch (device float32 pointers, contiguous). */
int td3_train_step_batch(td3_handle* h, const float* state, const float* action,
                         const float* next_state, const float* reward, const float* not_done,
                         int batch, void* stream, const float* inject_noise,
                         td3_step_stats* stats);
/* n states (host, [n][sd]) -> n actions (host, [n][ad]); synchronous.  Ordered after the last queued
 * step that updates the online actor (run in that step's stream when it is the handle's own, else
 * behind an event recorded on the caller's stream), not after critic-only steps: those it overlaps. */
int td3_select_action(td3_handle* h, const float* state, float* action_out, int n);
/* (state, action) (host) -> q_out[2*n] = Q1, Q2; synchronous. */
int td3_eval_q(td3_handle* h, const float* state, const float* action, float* q_out, int n);

/* Device-resident queries (these two: featured learners; a particle handle returns -1 and has
 * td3_select_action_particles_device / td3_eval_q_particles_device below).  Nothing crosses the
 * host: rows are read from and written to device memory, the call only queues work.
 * Exploration noise applied on the device (main.py:249-252, utils/noise.py).  The N(0,1) values are
 * Philox4x32-10 with key (seed lo, seed hi) and counter (idx, stream id, step lo, step hi), where
 * idx = row * ceil(action_dim / 4) + column / 4 (four normals per counter) and the stream id is the
 * exploration draw's own (4), not the one of the training step's target-policy noise (2): the same
 * (seed, step) gives unrelated values in the two. */
typedef struct td3_explore {
  float* x;                       /* device [n][ad] OU state, read and written; NULL: Gaussian, a = clip(pi + sigma*z) */
  float mu, theta, sigma;         /* X <- X + (theta*(mu - X) + sigma*z); a = clip(pi + X, -max_action, max_action) */
  const uint8_t* reset;           /* device [n], nullable: nonzero -> X = mu before this update (episode ended) */
  uint64_t seed, step;            /* Philox key / counter of this call's N(0,1) draw */
  const float* inject_z;          /* device [n][ad], nullable: replaces the draw (parity testing) */
  float* z_out;                   /* device [n][ad], nullable: receives the N(0,1) values used */
} td3_explore;
/* device state [n][sd] -> device action_out [n][ad]; ex NULL: the plain policy.  Any n >= 1 (the first
 * call at a new pad32(n) builds its plan, which synchronises the device once).  Asynchronous on `stream`
 * (NULL: the learner's step stream, so it is ordered after every queued step); no host synchronisation.
 * A non-NULL stream is first ordered after the last queued step's stream, and after a previous device
 * query on another stream, by an event recorded there: a caller's stream given to a step or to a
 * device query must stay alive until the next device query or td3_destroy.  A step queued LATER on
 * another stream is not ordered after the query: the caller orders those.  Pointers must stay valid
 * until the stream's work has completed. */
int td3_select_action_device(td3_handle* h, const float* state, int n, const td3_explore* ex,
                             float* action_out, void* stream);
/* device (state, action) -> device q_out [2][n] (Q1 then Q2); asynchronous as above. */
int td3_eval_q_device(td3_handle* h, const float* state, const float* action, int n, float* q_out, void* stream);

/* TD3_particles (TD3_particles.py:153-164, 167-224). */
int td3_train_step_batch_particles(td3_handle* h, const float* feat, const float* part, const float* action,
                                   const float* next_feat, const float* next_part, const float* reward,
                                   const float* not_done, int batch, void* stream, const float* inject_noise,
                                   td3_step_stats* stats);
/* TD3_particles.TD3._actor_learn(state_features, state_particles) (TD3_particles.py:209-224), as
 * evaluate_model.py:39-49 calls it outside train(): -mean Q1(s, pi(s)) with the current critic, the
 * actor's Adam step (its step counter only; total_it unchanged), Polyak of critic and actor.
 * feat [batch][F] / part [batch][N][D]: device float32, contiguous.  actor_loss (nullable, forces a
 * sync) receives the loss value. */
int td3_actor_learn_particles(td3_handle* h, const float* feat, const float* part, int batch, void* stream,
                              double* actor_loss);
/* host feat [n][F], part [n][N][D] -> action_out [n][A] (tanh policy) */
int td3_select_action_particles(td3_handle* h, const float* feat, const float* part, float* action_out, int n);
/* -> q_out [2][n][A] (Q1, then Q2; Q2 = Q1 when CDQ is off) */
int td3_eval_q_particles(td3_handle* h, const float* feat, const float* part, const float* action, float* q_out,
                         int n);
/* The same two queries on DEVICE rows (feat [n][F], part [n][N*D], action [n][A], all contiguous
 * float32), asynchronous and ordered exactly as td3_select_action_device (stream, events, plan per
 * pad32(n), any n >= 1).  The particle rows are not copied: the encoder reads `part` in place, and
 * nothing outside [n][N*D] is read.  A featured handle returns -1.
 * select: action_out [n][A] = clip(tanh policy + noise, -max_action, max_action) with `ex` as for
 * td3_select_action_device (same td3_explore, same Philox stream id); ex NULL: the plain tanh policy. */
int td3_select_action_particles_device(td3_handle* h, const float* feat, const float* part, int n,
                                       const td3_explore* ex, float* action_out, void* stream);
/* -> device q_out [2][n][A]: Q1 then Q2; Q2 = Q1 without CDQ. */
int td3_eval_q_particles_device(td3_handle* h, const float* feat, const float* part, const float* action,
                                int n, float* q_out, void* stream);

/* ------------------------------------------------------------------ training log */
/* Per-step losses and Q statistics of the learner, kept on the device (no counterpart in the reference;
 * what a host loop would print from the loss tensors of TD3.train).  td3_step_stats reports them too, but
 * stops the queue on every step; the log is a ring of `capacity` td3_log_entry in device memory, written
 * by ONE extra launch per logged step (train_log_kernel: one workgroup of 256 threads) and read when the
 * caller chooses.  A learner without the log queues nothing new: its steps stay bit for bit what they are.
 * The log belongs to the handle, not to the step plan: a rebuild at another batch size keeps it, and every
 * entry records its own `batch`.
 *
 * Which steps log: the log is enabled, total_it after the step is a multiple of `every`, and the call is
 * td3_train_step, td3_train_step_batch, td3_train_step_batch_particles, td3_train_step_prioritized or
 * td3_train_step_prioritized_particles (td3_probe_kernel's steps are td3_train_step calls and log).
 * td3_actor_learn_particles (no critic step) and the step of td3_profile_stages never log.  Logged step
 * number k = 0, 1, ... (the sequence number) goes to slot k mod capacity; `count` is the number logged so far.
 * The launch is queued on the step's stream directly behind the step's body -- in a prioritized step behind
 * the combine and the priority write-back -- and before the synchronisation a non-null `stats` forces.  It
 * is always a direct launch, never part of a captured graph: the sequence number, `step` and the flags are
 * kernel arguments the host knows, so the log needs no device counter and no atomics.
 *
 * The kernel reads only rows r < B of the step's buffers, never a pad row: y and Q1 ([B][nq], nq = 1 for a
 * featured learner, action_dim for a particle learner); Q2 where the learner has a twin (featured learners
 * always, particle learners with CDQ); the rows' squared errors of each critic as the loss rows wrote
 * them (on prioritized steps weighted); Q1(s, pi(s)) on actor steps; the importance weights on prioritized
 * steps.  All arithmetic is fp64 on the fp32 values widened, in one fixed order, so entries repeat bit
 * for bit: the elements e = r * nq + o are numbered 0 .. B*nq - 1; thread p accumulates e = p, p + 256, ...
 * in increasing order starting from 0.0; the 256 partials are combined through LDS by a halving tree
 * (partial[p] += partial[p + s], s = 128, 64, ..., 1, rs_tick_kernel's tree); quantities per row use the
 * same scheme over the rows r; min and max use the same partition and tree with < and >, threads without
 * an element carrying +inf / -inf; a mean is the tree's sum divided once by the count.  Nothing is
 * contracted into an fma: the only products are by 0.5 and 1 / (J*A), applied to a row's value before it
 * enters a sum.  With n = B * nq, J critics (2 with a twin, else 1) and A = nq:
 *   critic_loss   S_1 / n + S_2 / n, S_j the sum over rows of critic j's squared-error row (the second
 *                 term only with a twin): td3_step_stats.critic_loss's formula, the weighted loss on
 *                 prioritized steps
 *   actor_loss    -(sum of Q1(s, pi(s))) / n on actor steps, NaN otherwise
 *   q1_mean, q2_mean, y_mean; q_min, q_max over both critics; y_min, y_max
 *   q_gap_mean    the mean of |Q1 - Q2| over the elements
 *   td_abs_mean, td_abs_max   over the rows of t_r = 1/(J*A) sum_j sum_o |Q_j,r,o - y_r,o|, o in
 *                 increasing order, the critics then added in order j (featured: 0.5 (|Q1 - y| + |Q2 - y|))
 *   w_mean, w_min over the rows' importance weights on prioritized steps; exactly 1.0 otherwise, written
 *                 without reading the buffer
 *   nonfinite     the number of non-finite elements among y, Q1 and (with a twin) Q2
 * Without a twin the q2 values repeat Q1's and q_gap_mean is 0.  Where nonfinite > 0 the other fields are
 * whatever IEEE arithmetic gives; only nonfinite itself is specified.
 *
 * td3_log_enable: allocates the ring.  Data-parallel logging is out of scope: a handle in a td3_comm_init /
 *   td3_comm_init_local group is refused, and both of those return -1 on a handle whose log is enabled.
 * td3_log_info: a handle without the log reports enabled = 0 (and returns 0: this is the query for it).
 * td3_log_read: rs_read_episodes' semantics -- the entries with sequence numbers in [first, first + n) that
 *   are still in the ring (the last `capacity`), oldest first, into out; *first_out is the sequence number
 *   of out[0], *n_out the entries written.  Synchronous: it waits for an event recorded behind the last
 *   log launch (not for a stream: a caller's stream may be gone by then).
 * td3_log_set: restores the last n <= capacity entries (sequence numbers count - n .. count - 1) and the
 *   total `count`, for checkpoints; synchronous.  A run continued after it reads back exactly what the
 *   uninterrupted run does.
 * Checked in this order, each failure returning -1 before any GPU work with a message naming the field:
 *   td3_log_enable: capacity in 1..2^20; every in 1..2^20; the handle; not already enabled; not in a
 *     td3_comm_init or td3_comm_init_local group.
 *   td3_log_read: first >= 0; n >= 0; out non-null unless n == 0; first_out; n_out; the handle; enabled.
 *   td3_log_set: n >= 0; entries non-null unless n == 0; count >= n; the handle; enabled; n <= capacity.
 *   td3_log_info: info non-null; the handle. */
typedef struct td3_log_entry {
  int64_t step;            /* total_it after the step */
  int32_t batch;           /* B of the step */
  int32_t actor_step;      /* 1 when the delayed policy update ran */
  int32_t prioritized;     /* 1 for td3_train_step_prioritized(_particles) */
  int32_t nonfinite;
  double critic_loss, actor_loss;
  double q1_mean, q2_mean, y_mean;
  double q_min, q_max, y_min, y_max;
  double q_gap_mean;
  double td_abs_mean, td_abs_max;
  double w_mean, w_min;
} td3_log_entry;
typedef struct td3_log_info_t {
  int enabled, capacity, every;
  int64_t count;           /* steps logged so far (the next sequence number) */
} td3_log_info_t;
/* sizeof(td3_log_entry) of this library: a binding checks its own struct against it. */
size_t td3_log_entry_size(void);
int td3_log_enable(td3_handle* h, int capacity, int every);
int td3_log_info(const td3_handle* h, td3_log_info_t* info);
int td3_log_read(td3_handle* h, int64_t first, int64_t n, td3_log_entry* out, int64_t* first_out,
                 int64_t* n_out);
int td3_log_set(td3_handle* h, const td3_log_entry* entries, int64_t n, int64_t count);

/* ------------------------------------------------------------------ TD3+BC (offline data) */
/* The behaviour-cloning term of TD3+BC (Fujimoto & Gu 2021, "A Minimalist Approach to Offline
 * Reinforcement Learning") in the actor step of a featured learner, every norm, one device.  The
 * reference's workflow it serves: a buffer filled from a recorded policy (experience_injection.py) and
 * main.py --load_replay_buffer, which trains on the loaded rows from the first tick.  On a step whose
 * delayed policy update runs, with alpha > 0, B rows, A = action_dim, pi_r = max_action tanh(z4_r) as the
 * step's actor forward computed it, a_r the batch's stored action and Q_r = Q1(s_r, pi_r) with the critic
 * as the step's critic update left it:
 *   q_abs_mean = 1/B sum_r |Q_r|                        (no gradient flows through it)
 *   lambda     = alpha / q_abs_mean
 *   loss       = -lambda 1/B sum_r Q_r + 1/(B*A) sum_r sum_o (pi_r,o - a_r,o)^2
 *   dL/dpi_r,o = lambda g_r,o + 2/(B*A) (pi_r,o - a_r,o)
 * g_r,o is dQ1/da_o of the plain step (through Q1's layer 0, carrying -1/B).  Everything behind dL/dpi is
 * the plain step's: tanh backward, the actor head, LN3 backward, the input-grad stages, dW, Adam, Polyak.
 * The critic phase is untouched; in td3_train_step_prioritized the importance weights still touch only
 * the critic.  All of it is float32 on the device: sum_r |Q_r| runs over the rows r < B only, never a pad
 * row, in one fixed order (lane l of one wave adds rows l, l + 64, ... ascending from 0.0f, the 64
 * partials through the wave's fixed reduction tree), divided once by (float)B; lambda = (float)alpha /
 * that.  Every wave that needs lambda uses those bits, whatever the grid, the head path (narrow / wide)
 * or the launch mode (graph / direct).  q_abs_mean == 0 gives lambda = inf as the paper's code does:
 * there is NO guard.  Each row's sum_o (pi - a)^2 is added in increasing o.
 * The stored action is read from the step's [s | a] batch rows, which every input path fills (ring sample
 * fused into the first layer or gathered, injected indices, td3_train_step_batch).
 *
 * td3_set_bc: alpha = 0 turns the term off.  Synchronises the learner and, when alpha changes, rebuilds
 *   the step plan and its captured graphs (alpha, B and A are launch arguments; lambda itself is computed
 *   on the device, so the graphs replay unchanged).  With alpha == 0, or on a handle never touched, the
 *   step is exactly the plain one: the same stage list, the same kernels, the same bits.  With alpha > 0
 *   the actor phase runs the BC form of the actor_head_bwd stage (td3_stage_kernel names it); nothing
 *   else in the stage list changes.  Every single-device featured step entry point takes it:
 *   td3_train_step, td3_train_step_batch, td3_train_step_prioritized, td3_probe_kernel,
 *   td3_profile_stages.
 *   Returns -1 with a message, before any GPU work, for (checked in this order): alpha negative or
 *   non-finite; a null handle; a particle handle (the particle learner has no BC step yet); a handle in a td3_comm_init or
 *   td3_comm_init_local group -- and both of those refuse a handle with BC on: lambda would need the
 *   global batch's mean.
 * td3_step_stats.actor_loss and the training log's actor_loss keep their meaning with BC on:
 *   -mean Q1(s, pi(s)), not the BC loss.  No struct layout changes.
 * td3_bc_info: synchronous; with a BC step to report it waits for the whole device (hipDeviceSynchronize: that
 *   step may sit on a caller's stream the handle no longer knows to be alive).  `step` is total_it of the last actor
 *   step taken with BC in the current step plan, 0 if none (a plan rebuild -- td3_set_bc, another batch
 *   size, td3_set_adam -- forgets it); lambda and q_abs_mean are that step's float32 values widened;
 *   bc_loss = (sum over r < B, in row order, of the row sums widened to fp64) / (B*A).  With step == 0
 *   the three are 0.  Returns -1 for a null info, then a null handle. */
typedef struct td3_bc_info_t {
  int enabled;
  double alpha;
  int64_t step;
  double lambda, q_abs_mean, bc_loss;
} td3_bc_info_t;
int td3_set_bc(td3_handle* h, double alpha);
int td3_bc_info(td3_handle* h, td3_bc_info_t* info);

/* ------------------------------------------------------------------ Demonstration replay (two rings) */
/* One TD3.train step of either learner kind, on one device, whose batch rows [0, n_demo) come from the
 * ring `demo` and rows [n_demo, batch) from the ring `rb` ("symmetric sampling": Vecerik et al. 2017,
 * DDPGfD; Ball et al. 2023, RLPD).  The reference's workflow it serves: a buffer filled from a recorded
 * policy (experience_injection.py) kept as `demo`, and online training on top of it (main.py
 * --load_replay_buffer) adding to `rb`, so the demonstrations' share of a batch neither decays nor is
 * overwritten by the FIFO.  Both rings have the learner's kind and dims, hence one record layout.
 *
 * The draw of batch row r is uniform on r's own ring: philox_index(seed of that ring, total_it + 1, r,
 * size of that ring) -- td3_train_step's draw with the batch row as counter on both sides.  n_demo = 0 is
 * td3_train_step's draw on `rb`, n_demo = batch its draw on `demo`, and both equal that step bit for bit.
 * One input launch (csrc/mixed.hip) fills the plan's batch buffers from both rings -- for a particle
 * learner also the packed particle rows [Bp][2 N D] (s | s') its encoders then read, as in
 * td3_train_step_batch_particles -- and the step's body is the one of the injected-index steps.  n_demo
 * is an argument of that launch alone: it may change every step with no plan rebuild and no re-capture.
 *
 * inject_idx: host [batch], nullable; its first n_demo entries index `demo`, the rest `rb`, each checked
 *   against its ring's capacity.  inject_noise, stats (stats->idx: the drawn rows, each in its own ring),
 *   the host synchronisations they force, the counters, the training log (prioritized = 0), TD3+BC (its
 *   term covers every row of the batch unless td3_set_bc_filter narrows it) and gradient clipping are td3_train_step's.
 * Ordering: the step is ordered after every add queued on either ring before it, and adds to either ring
 *   queued after it wait for its reads (one read section on `rb`, then `demo`).
 * Mixing step kinds: a mixed step after a prioritized one refills unit weights; a plain or prioritized
 *   step after a mixed one is bit for bit what it would have been (a particle learner's encoders switch
 *   back to the ring, as after td3_train_step_batch_particles).
 * Returns -1 with a message, before any GPU work and leaving the counters and both rings' ordering state
 *   unchanged, for (checked in this order): batch <= 0; n_demo outside [0, batch]; a null h, rb or demo;
 *   rb == demo; a ring whose kind, dims, particle shape or device do not match the learner (rb, then
 *   demo); priorities enabled on either ring (the mixed draw is uniform); a handle in a td3_comm_init /
 *   td3_comm_init_local group; a ring that contributes at least one row being empty while inject_idx is
 *   null (a ring that contributes no row may be empty); an injected index outside its ring.
 * td3_debug_mixed_input: re-queues the last mixed step's input launch on the rows that step read
 *   (measurement); -1 unless the handle's last step was a mixed step on these two rings in the current
 *   step plan.  No struct layout changes. */
int td3_train_step_mixed(td3_handle* h, rb_handle* rb, rb_handle* demo, int batch, int n_demo, void* stream,
                         const int64_t* inject_idx, const float* inject_noise, td3_step_stats* stats);
int td3_debug_mixed_input(td3_handle* h, rb_handle* rb, rb_handle* demo, void* stream);  /* re-queue the last mixed step's input launch (measurement) */

/* ------------------------------------------------------------------ BC on the demonstration rows, Q-filter */
/* Which rows of the batch the TD3+BC term covers (Nair et al. 2018, "Overcoming Exploration in Reinforcement
 * Learning with Demonstrations", §IV-B/C): the rule for fine-tuning on top of demonstrations, the workflow
 * td3_train_step_mixed exists for.  td3_set_bc alone is the offline rule (every row of the batch is data to
 * imitate); on a mixed batch that also pulls pi(s) toward the learner's own old, noise-perturbed actions in
 * the online rows.  Two switches, each 0 or 1, both 0 being exactly the step of "TD3+BC" above.  A featured
 * learner, one device, every norm, a step whose delayed policy update runs with alpha > 0; B, A, pi_r, a_r,
 * g_r,o and lambda as in "TD3+BC" -- lambda = alpha / mean over ALL B rows of |Q1(s_r, pi_r)|, unchanged:
 *   n_d    = the step's n_demo if demo_rows (td3_train_step_mixed: its n_demo argument; every other step
 *            kind: B -- a step that draws from one ring has no online rows), else B
 *   cand_r = r < n_d
 *   keep_r = cand_r and (not q_filter or Q1sa_r > Q1pi_r)        strict >, a float32 compare: a NaN on
 *            either side drops the row
 *            Q1sa_r = Q1(s_r, a_r) as this step's critic phase computed it: the critic BEFORE this step's
 *                     update, the value in the step's TD error (td3_step_stats.q1)
 *            Q1pi_r = Q1(s_r, pi_r) as the actor phase computes it: the critic AFTER the update
 *   dL/dpi_r,o = lambda g_r,o + keep_r c (pi_r,o - a_r,o),       c = (float)(2.0 / ((double)n_d * A))
 *   bc_loss    = sum_{r<B} keep_r sum_o (pi_r,o - a_r,o)^2 / (n_d A)       (0 when n_d = 0)
 *   kept       = sum_{r<B} keep_r
 * The two Q values come from critics one Adam step apart, on purpose: Q1(s, a) of the updated critic would
 * cost a second Q1 forward per actor step, and the filter asks which of two actions the critic rates
 * higher, which one step of Adam rarely changes.  The term is normalised by the candidate count n_d, not
 * by kept, also on purpose: it weakens as the filter drops rows and fades once the policy overtakes the
 * demonstrator.  With n_d = 0 no row is a candidate, c is never used and the step is lambda-scaled TD3.
 * With n_d = B, c is the constant of "TD3+BC" bit for bit, and with every row kept so is the step.
 * Everything behind dL/dpi is the plain step's; the critic phase is untouched; importance weights of a
 * prioritized step still touch only the critic.
 *
 * On the device: a third form of the actor_head_bwd row stage (csrc/bcf.hip, td3_stage_kernel names it
 * td3::row_bcf_kernel); nothing else in the stage list changes.  Each row's wave decides keep_r itself and
 * forms c in float64 from n_d, once; a row that is not kept writes 0 as its squared error and adds no BC
 * term.  No reduction beyond lambda's, no atomics.  n_d is a 4-byte device word the step plan owns: with
 * demo_rows on, every actor step of td3_train_step, td3_train_step_batch, td3_train_step_prioritized
 * (each n_d = B; td3_profile_stages and td3_probe_kernel too) and td3_train_step_mixed (n_d = n_demo)
 * queues a 4-byte write of it on the step's stream ahead of the step's body, outside every captured
 * graph, so n_demo may change every step with no plan rebuild and no re-capture.  With demo_rows off
 * nothing is queued: the word holds B from the plan's build.
 *
 * td3_set_bc_filter: stores the switches; while alpha > 0 a changed switch synchronises the learner and
 *   rebuilds the step plan and its captured graphs (as td3_set_bc does).  With alpha == 0 they wait for
 *   td3_set_bc; with both 0 the learner is the one never touched: the same stage lists, kernels and bits.
 *   Returns -1 with a message, before any GPU work, for (checked in this order): a switch that is not 0 or
 *   1; a null handle; a particle handle; a handle in a td3_comm_init / td3_comm_init_local group.
 * td3_bc_filter_info: synchronous like td3_bc_info.  `step` is total_it of the last actor step taken with
 *   the filtered form in the current step plan, 0 if none (a plan rebuild forgets it), and then n_demo,
 *   kept and bc_loss are 0.  n_demo is that step's n_d; kept and bc_loss are summed on the host from the
 *   rows' keep flags and squared errors, in row order, in float64.  td3_bc_info.bc_loss reports the same
 *   masked value on such a step.  Returns -1 for a null info, then a null handle.
 * td3_bc_filter_keep: that step's keep_r as 0.0f / 1.0f, host keep[n], n = its batch size; synchronous;
 *   -1 without such a step.  No existing struct changes. */
typedef struct td3_bc_filter_info_t {
  int demo_rows, q_filter;
  int64_t step;
  int64_t n_demo, kept;
  double bc_loss;
} td3_bc_filter_info_t;
int td3_set_bc_filter(td3_handle* h, int demo_rows, int q_filter);
int td3_bc_filter_info(td3_handle* h, td3_bc_filter_info_t* info);
int td3_bc_filter_keep(td3_handle* h, float* keep, int n);

/* ------------------------------------------------------------------ gradient clipping */
/* torch.nn.utils.clip_grad_norm_ with its defaults (norm_type = 2, error_if_nonfinite = False) between a
 * group's backward and its Adam step, on one device.  The rule is per group: the critic group is both
 * twins and, on a particle learner, their encoders (critic.parameters()); the actor group includes its
 * encoder.  Each optimizer step of a group with max_norm > 0 does
 *   total = sqrt(sum over every parameter element of g^2)
 *   coef  = min(1, max_norm / (total + 1e-6))
 *   Adam sees coef * g
 * with NO guard for a non-finite total: IEEE arithmetic decides, as in torch (a NaN total gives a NaN coef).
 * Arithmetic: every fp32 gradient element is widened and squared in fp64 and accumulated in fp64 in one
 * fixed order that depends on the arena's size alone (DESIGN.md §4b spells it) -- not on the batch, the
 * launch mode or the dW kernel that produced the gradient; sqrt, the sum with 1e-6, the division and the
 * min are fp64; coef is rounded to fp32 once and multiplies g in fp32.  No float atomics: runs repeat bit
 * for bit, and graph replay equals direct launches.  The gradient arena itself is not scaled:
 * td3_get_params(TD3_*_GRAD) of a clipping group returns the step's unclipped batch-mean gradient.
 *
 * A clipping group takes, in place of its fused <tag>_dw stage (tag C / A): <tag>_dw in gradient-only mode
 * (and <tag>_enc_adam likewise, particles), <tag>_gnorm (one launch: W workgroups, one fp64 partial each)
 * and <tag>_adam (the flat Adam pass with Polyak and the forward weights' images; every workgroup adds the
 * W partials in index order and forms coef itself).  A group without clipping keeps its fused stage:
 * clipping the critic only leaves the actor phase exactly as it is.  A handle never touched, or set back
 * to 0, runs the same stage list, the same kernels and the same bits as without the feature.
 * Taken by featured learners with norm None or "layer" and particle learners (CDQ on and off), on every
 * single-device step entry point, with TD3+BC on or off: td3_train_step, td3_train_step_batch,
 * td3_train_step_batch_particles, both prioritized steps (the norm is of the weighted gradient),
 * td3_actor_learn_particles (the actor group), td3_probe_kernel, td3_profile_stages.
 *
 * td3_set_grad_clip: group 0 actor, 1 critic (td3_set_adam's convention); max_norm = 0 turns the group's
 *   clipping off.  It waits for the learner's queued steps.  max_norm lives in a device scalar: changing
 *   one positive value to another rebuilds nothing (the captured graphs replay unchanged; anneal it
 *   freely); switching a group on or off rebuilds the step plan and its graphs, as td3_set_bc does.
 *   Returns -1 with a message, before any GPU work, for (checked in this order): max_norm negative or
 *   non-finite; group not 0 or 1; a null handle; a weight-normalised learner (norm: its Adam runs on
 *   dg / dv inside wn_kernel); a handle in a td3_comm_init or td3_comm_init_local group -- and both of
 *   those refuse a handle with clipping on (the data-parallel form is the norm behind the all-reduce).
 * td3_clip_info: synchronous like td3_bc_info.  step[g] is total_it of group g's last optimizer step taken
 *   with clipping in the current step plan (td3_actor_learn_particles does not move total_it and reports
 *   under the current one), grad_norm[g] that step's total before scaling, coef[g] the float32 factor the
 *   kernel used, widened.  A plan rebuild forgets the three (0).  Returns -1 for a null info, then a null
 *   handle.  No other struct changes its layout. */
typedef struct td3_clip_info_t {
  int     enabled[2];     /* index = group: 0 actor, 1 critic (td3_set_adam's convention) */
  double  max_norm[2];
  int64_t step[2];        /* total_it of the group's last optimizer step taken with clipping in the current plan, 0 if none */
  double  grad_norm[2];   /* that step's total L2 norm of the group's gradient, before scaling */
  double  coef[2];        /* the factor applied, as the float32 the kernel used, widened */
} td3_clip_info_t;
int td3_set_grad_clip(td3_handle* h, int group, double max_norm);   /* 0 turns the group's clipping off */
int td3_clip_info(td3_handle* h, td3_clip_info_t* info);

/* ------------------------------------------------------------------ multi-GPU (RCCL) */
int td3_comm_unique_id(unsigned char out[128]);
/* Data-parallel mode: grads are all-reduced (sum, then /world) over RCCL before Adam.  Every
 * call that steps the learner is then COLLECTIVE: td3_train_step / td3_train_step_batch and
 * td3_actor_learn_particles must be made by every rank in the same order (each issues the
 * phase all-reduces).  With TD3_DP_BUCKETS=1 in the environment when the plan is built, a twin
 * critic at B >= 512 exchanges its gradients per network, bucket 0 on a comm stream under
 * bucket 1's dW (off by default: measured slower on one rank). */
int td3_comm_init(td3_handle* h, const unsigned char id[128], int nranks, int rank);
/* The data-parallel optimizer step is the all-reduce + replicated Adam by default; TD3_DP_SHARD in the
 * environment when the plan is built selects the SHARDED form (1: for nranks > 1, 2: even at one rank;
 * weight normalization and TD3_DP_BUCKETS=1 keep the all-reduce): ncclReduceScatter of the gradient, Adam on this rank's 1/nranks slice,
 * ncclAllGather of the parameters, replicated Polyak.  Parameters and targets stay identical on
 * every rank; the Adam moments of slice k live on rank k.  Reading the moments (td3_get_params
 * with TD3_*_ADAM_M / _V, e.g. a checkpoint) then needs this COLLECTIVE first, on every rank, after
 * the last step (a td3_comm_init_local replica consolidates by itself).  Replaces nothing in the
 * reference: torch.optim.Adam.state_dict (TD3_base.py:26-34 saves it) on a sharded optimizer. */
int td3_dp_gather_optimizer_state(td3_handle* h);
/* Test seam of the same data-parallel path inside ONE process (RCCL cannot put two ranks on one
 * GPU): the n handles (same configuration and device) become the ranks 0..n-1 of a group whose
 * all-reduce is a fixed-order device sum over their G arenas.  Their plans switch to the
 * data-parallel stage lists exactly as td3_comm_init does (grad-only dW, all-reduce, flat Adam with
 * grad_scale 1/n, Polyak); they step together through td3_train_step_local only. */
int td3_comm_init_local(td3_handle** hs, int n);
/* One TD3.train step of every replica of a td3_comm_init_local group, stage by stage on rank 0's
 * stream; replica k samples rbs[k].  inject_idx [n][batch] / inject_noise [n][batch][ad] (host,
 * nullable) as td3_train_step; stats [n] (nullable). */
int td3_train_step_local(td3_handle** hs, rb_handle** rbs, int n, int batch, const int64_t* inject_idx,
                         const float* inject_noise, td3_step_stats* stats);

/* ------------------------------------------------------------------ measurement */
/* Block until the learner stream's queued work is done (hipStreamSynchronize). */
int td3_sync(td3_handle* h);
void* td3_stream(td3_handle* h);
/* Per-stage device times (ms) of one eager step; names via td3_stage_name. */
int td3_profile_stages(td3_handle* h, rb_handle* rb, int batch, int actor_phase, float* ms,
                       int max_stages, int* n_stages);
const char* td3_stage_name(td3_handle* h, int i);
/* HIP kernel function launched by stage i (the name rocprofv3 reports). */
const char* td3_stage_kernel(td3_handle* h, int i);
/* Debug: stage i of the stage list the handle's last step ran (td3_train_step_local records it, as
 * td3_profile_stages does; a rebuilt plan forgets it): its name, or with `kernel` != 0 its HIP kernel.
 * "" out of range -- the list ends there.  A td3_comm_init_local replica cannot run
 * td3_profile_stages (its collective stages refuse to launch); this reads what its step left. */
const char* td3_debug_last_stage(td3_handle* h, int i, int kernel);
/* Re-launch one stage `iters` times back-to-back (captured in one hipGraph, replayed between
 * two HIP events on the handle stream, after one full step at `batch`); returns mean ms per
 * launch.  Stage 0 is the stand-alone replay-ring gather (gather_kernel) of the profiled ring. */
int td3_time_stage(td3_handle* h, int stage, int iters, float* ms_mean);
/* Run `steps` production training steps (Philox draws from rb, direct launches) with every launch
 * of the HIP kernel `kernel` (a td3_stage_kernel name) between two HIP events on the step stream:
 * the kernel's in-step device time, summed over its `launches`.  Real steps: counters and
 * parameters advance. */
int td3_probe_kernel(td3_handle* h, rb_handle* rb, int batch, const char* kernel, int steps, float* ms_total,
                     int* launches);
/* Algorithmic FLOPs of one launch of stage i (MFMA stages; 0 otherwise). */
double td3_stage_flops(td3_handle* h, int i);
/* Algorithmic HBM bytes of one launch of stage i (operands and results once, optimizer state per
 * parameter; 0 where not accounted): the bytes side of SURVEY §8d's roofline. */
double td3_stage_bytes(td3_handle* h, int i);
/* Test instrumentation: the post-ReLU activations H_layer (layer 0..2) of one network evaluation of the
 * last featured train step, rows x cols (cols <= the layer's width) into out (host, row-major).  eval:
 * 0 target actor (s'), 1 Q1 (s, a), 2 Q2 (s, a), 3 actor (s), 4 / 5 target Q1 / Q2 (s', a'), 6 Q1 (s, pi).
 * The tests take the ReLU masks of the step from it: where a pre-activation lies within fp32 rounding of
 * zero the oracle and the GPU may both be right about opposite masks (tests/test_gpu_gradients.py). */
int td3_debug_activation(td3_handle* h, int eval, int layer, float* out, int rows, int cols);
/* Test instrumentation: properties of the current step plan (0 before the first step): bit 0 = the forward
 * GEMM stages read the k-quad weight images (learner.h Group::P4 / T4; TD3_W4 != 0, every featured plan
 * except weight normalization -- any batch size, data-parallel plans included; particle learners never),
 * bit 1 = the plan's optimizer steps are sharded over ranks.  A rebuild that leaves a sharded schedule
 * gathers the Adam moments first (collective on RCCL ranks, as td3_dp_gather_optimizer_state). */
int td3_debug_plan_flags(const td3_handle* h, int* flags);
/* Measurement instrumentation (tools/bench_per.py): queue on `stream` one stage of the last prioritized
 * step of this handle on this ring, over the rows that step drew (the plan's buffers still hold them):
 * stage 0 the gather of those rows into the batch buffers, inside a read section of its own; stage 1 the
 * particle step's combine of the critics' |TD error| rows (a featured step has none: -1).  -1 before the
 * first prioritized step of the current plan on this ring.  The draw and the priority update are
 * rb_sample_prioritized and rb_update_priorities themselves. */
int td3_debug_per_stage(td3_handle* h, rb_handle* rb, int stage, void* stream);
/* Measurement instrumentation (tools/bench_train_log.py): queue on `stream` the training log's launch of
 * the last logged step once more, over the plan's buffers as that step left them and into the same slot
 * (the entry is rewritten with the same values; count does not move).  -1 unless the last step of this
 * handle was logged. */
int td3_debug_log_launch(td3_handle* h, void* stream);

/* Test seam of the one-launch query's failure path: in the next n select_action / eval_q launches
 * (existing query plans) workgroup 0 acts as if its in-launch layer-1 poll had timed out.  The query
 * must then fail (rc < 0, the kernel publishes its flag with the failure bit) and the next query must
 * be correct again (the host re-zeroes the hand-off counters). */
int td3_debug_act_fail(td3_handle* h, int n);
/* Test instrumentation: which route a featured query of n rows takes (eval_q != 0: td3_eval_q, else
 * td3_select_action; device != 0: their _device forms), written into buf (len bytes, NUL-terminated) as a
 * comma-separated list.  The first token says where the query's rows travel: "args" (in the kernel
 * arguments), "mapped" (mapped host memory) or "device" (device scratch); the rest are the HIP kernels the
 * query would launch, in order, named as td3_stage_kernel names them, e.g.
 * "args,td3::act_kernel<4, 16>" or "args,td3::gemv01_kernel<2>,td3::gemv_kernel<2>,td3::head_kernel".
 * A query that runs a plan's stage list gives the stages' kernels (the device forms' row packing in front
 * of the list and their exploration epilogue behind it are not named).  Builds the query plan of pad32(n)
 * rows if it does not exist yet; launches nothing.  The answer comes from the function the queries
 * themselves dispatch on. */
int td3_debug_query_route(td3_handle* h, int n, int eval_q, int device, char* buf, int len);
/* Test seam of the wide heads (action width > 8): the dynamic LDS bytes of the calling thread's last row-kernel
 * launch, i.e. of the weight rows its workgroups staged (0: every head was requested block by block, e.g.
 * under TD3_WIDE_HEADS=0; -1: no row launch yet).  Launches replayed from a captured graph do not count: use it
 * behind a direct launch (td3_profile_stages, use_graph = 0). */
int td3_debug_row_lds(void);

const char* td3_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TD3_HIP_H */
