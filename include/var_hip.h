/*
 * var_hip.h -- C ABI of libvar_hip.so, the MI355X (gfx950) implementation of the
 * VAR contrastive-pretext hot path of PeixinC/VoiceControlledRobot-VAR.
 *
 * The reference has no FFI: its seam is the class-valued config attribute
 * `config.pretextModel = VARPretextNet`
 * (Envs/pybullet/arms/tasks/fourInARow/config.py:30) and the torch calls made by
 * VAR_Pretext.trainRepresentation (VAR/pretext_VAR.py:55-70).  Each entry point
 * below names the reference code it stands in for.  INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. tensor.data_ptr());
 *     the library owns only its context workspace;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); entries are
 *     stream-ordered, never synchronise, never allocate (var_plan excepted) and are
 *     therefore capturable into a HIP graph;
 *   - return 0 on success, a negative VAR_ERR_* otherwise; var_last_error() gives text;
 *   - layouts are the reference's: images NCHW (u8 or f32), MFCC (B,1,100,40) f32,
 *     embeddings (B,3) row-major, parameters = the 26 state_dict() tensors of the Kuka
 *     VARPretextNet (models/pretext/arm_pretext_model.py:39-56) back to back in
 *     registration order, each in its PyTorch layout (OIHW / (out,in)): 213478 floats;
 *   - one context per (process, device); a context is not re-entrant.
 */
#ifndef VAR_HIP_H
#define VAR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAR_OK 0
#define VAR_ERR_ARG (-1)        /* bad argument (null pointer, unsupported size) */
#define VAR_ERR_HIP (-2)        /* a HIP runtime call failed */
#define VAR_ERR_PLAN (-3)       /* var_plan() not called or too small for this call */
#define VAR_ERR_STATE (-4)      /* backward without a saved forward, etc. */

#define VAR_N_PARAMS 213478
#define VAR_EMB_DIM 3
#define VAR_MFCC_FRAMES 100
#define VAR_MFCC_COEFFS 40

typedef struct var_ctx var_ctx;

/* Library / context -------------------------------------------------------- */

/* Create a context on `device_id` (replaces `model.to(device)`, pretext.py:306). */
int var_init(int device_id, var_ctx** out);
int var_destroy(var_ctx* ctx);
const char* var_last_error(var_ctx* ctx);   /* ctx may be NULL: last init error */
int var_param_count(void);                  /* == VAR_N_PARAMS */

/* Size the context workspace (activations, gradient scratch, split-K slabs) for up
 * to `max_batch` triplets of img_hw x img_hw images (84 or 96).  The only entry that
 * allocates; call it outside the step loop / graph capture. */
int var_plan(var_ctx* ctx, int max_batch, int img_hw);

/* Generation counters.  var_plan_generation: bumped by every re-plan (var_plan / var_ithor_plan growing the
 * workspace); a superseded workspace stays allocated until var_destroy, so HIP graphs captured against it keep
 * replaying on valid memory.  var_saved_generation: id (> 0) of the forward whose activations the workspace
 * currently holds for var_arm_encoder_bwd, 0 = none -- a host that interleaves forwards of several models
 * (autograd) compares it with the id it noted after its own forward before calling the backward. */
int var_plan_generation(var_ctx* ctx);
int var_saved_generation(var_ctx* ctx);

/* Kernel-side weight images, one per MODEL.  The kernels read conv filters re-laid as [tap][cin][cout] and
 * [tap][cout][cin] ("packed image", 1.2 MB) next to the parameter arena.  A host with several models on one
 * device -- the reference's RL stage keeps a frozen copy of the encoder beside the policy
 * (Envs/vec_env/vec_pretext_normalize.py:82-94) -- creates one image per model and binds it before that model's
 * calls; var_weights_bind(ctx, NULL) selects the context's own default image.  Binding is host state read at
 * launch time (like hipSetDevice): a captured graph keeps the image that was bound during capture.
 * var_pack_weights re-derives the BOUND image from `params` and records that arena; it must follow every change
 * of the parameters made outside this library (load_state_dict); var_adam_step* keep the bound image current by
 * themselves.  Every var_arm_* entry checks that the bound image was packed from the `params` it is given and
 * returns VAR_ERR_STATE otherwise. */
typedef struct var_weights var_weights;
int var_weights_create(var_ctx* ctx, var_weights** out);
int var_weights_destroy(var_ctx* ctx, var_weights* w);
int var_weights_bind(var_ctx* ctx, var_weights* w);
int var_pack_weights(var_ctx* ctx, void* stream, const float* params);

/* Encoder ------------------------------------------------------------------
 * PretextNetBase.VAR_forward (models/pretext/pretext_base.py:10-41) for the Kuka
 * VARPretextNet: imgBranch -> imgTriplet -> F.normalize, soundCNN -> soundTriplet ->
 * F.normalize for the positive and the negative clip.
 *   image            (B,C>=3,H,H) u8 or f32, first 3 channels used (pretext_base.py:22);
 *                    u8 images are divided by 255 as dataset.py:67-68 does; may be NULL
 *   image_bstride    elements between consecutive images (C*H*H)
 *   mfcc_pos/neg     (B,1,100,40) f32, either may be NULL
 *   outputs          any may be NULL: image_feat/pos_feat/neg_feat (B,3),
 *                    image_raw (B,576) = image_feat_raw, pos_raw (B,160) = pos_sound_raw
 *   save_for_bwd     1: keep activations in the workspace for var_arm_encoder_bwd; 0: do not; 2: do not, and a batch of
 *                    <= 64 images takes the kernels that minimise the latency of a small batch (the RL stage's 8 envs;
 *                    Envs/vec_env/vec_pretext_normalize.py:82-101) -- equal to the training forward within rounding, not bitwise
 */
int var_arm_encoder_fwd(var_ctx* ctx, void* stream, const float* params,
                        const void* image, int image_is_u8, long image_bstride,
                        const float* mfcc_pos, const float* mfcc_neg, int B, int H,
                        float* image_feat, float* pos_feat, float* neg_feat,
                        float* image_raw, float* pos_raw, int save_for_bwd);

/* out[r] = sum_k a[r][k] * b[r][k], rows x dim f32 (dim <= 64): the intrinsic reward <image_feat, goal_sound_feat> of
 * Envs/vec_env/vec_pretext_normalize.py:96-101 (`calcReward`: torch.sum(a * b, dim=1)) as ONE launch on `stream`; the sum
 * runs over k in index order in fp32. */
int var_row_dot(var_ctx* ctx, void* stream, const float* a, const float* b, int rows, int dim, float* out);
/* calcReward's embedding reward with config.RLRewardSoundSound on (vec_pretext_normalize.py:96-101), ONE launch on `stream`:
 *     a = sum_k image_feat[r][k] * goal_feat[r][k];  b = sum_k cur_feat[r][k] * goal_feat[r][k]      (var_row_dot's sums, fp32)
 *     out[r] = a + b (one fp32 add);  out_img[r] = a, out_snd[r] = b where those are not NULL
 * -- the reference's grouping: two float32 np.sum(axis=1), one float32 add; the float64 add of envReward is
 * var_reward_norm_step's, which takes `out` as its dot.  cur_feat = NULL drops the second term: out has var_row_dot's bits and
 * out_snd, where given, is 0.  rows x dim f32, dim <= 64.  VAR_ERR_ARG, nothing launched: image_feat / goal_feat / out NULL,
 * rows < 1, dim outside 1..64. */
int var_reward_dots(var_ctx* ctx, void* stream, const float* image_feat, const float* goal_feat,
                    const float* cur_feat /* NULL: no second term */, int rows, int dim, float* out,
                    float* out_img /* may be NULL */, float* out_snd /* may be NULL */);
/* var_reward_dots with the sound embeddings served from a device clip table (table_rows x dim f32: a clip's embedding is a constant
 * of the frozen checkpoint and the clip, Envs/audioLoader.py:166-237 draws from a finite, unaugmented pool), ONE launch, a thread
 * per row.  It follows an image-only var_arm_encoder_fwd(..., save_for_bwd = 2); var_set_reward_dot is not armed on this path.
 *   goal_ids (rows) i32 on the device | NULL: id g >= 0 takes table[g] and writes it to goal_feat[r] (the policy's
 *       goal_sound_feat); g == -1 reads goal_feat[r], the embedding cached FOR THAT ROW; NULL = every row -1.
 *   cur_ids (rows) i32 on the device | NULL: cur_feat[r] = table[c] and out = a + b, var_reward_dots' grouping; NULL: out = a,
 *       cur_feat untouched, out_snd (where given) 0.
 * An id outside its range (goal < -1 or >= table_rows; current < 0 or >= table_rows) is never turned into an address: that row's
 * out, out_img, out_snd and cur_feat are NaN and its goal_feat stays as it was; other rows are unaffected.  The ids are read on
 * the device, so one captured launch serves goal steps, cached steps and staggered resets.  VAR_ERR_ARG, nothing launched:
 * image_feat / table / goal_feat / out NULL, table_rows < 1, cur_ids without cur_feat, rows < 1, dim outside 1..64. */
int var_reward_dots_ids(var_ctx* ctx, void* stream, const float* image_feat, const float* table, int table_rows,
                        const int* goal_ids /* | NULL */, const int* cur_ids /* | NULL */, float* goal_feat /* in/out */,
                        float* cur_feat /* out | NULL */, int rows, int dim, float* out, float* out_img /* may be NULL */,
                        float* out_snd /* may be NULL */);
/* Arms the NEXT var_arm_encoder_fwd with an image: it also leaves reward_out[b] = <image_feat[b], goal_feat[b]> (3 floats per
 * row, var_row_dot's sum) -- the intrinsic reward of VAR/pretext_base.py's calcReward.  Where the image head is a launch of its
 * own that finishes the embeddings (save_for_bwd = 2, 84 x 84, at most 16 rows: the RL stage's envs) the dot rides in that launch
 * (each launch is ~5 us on that path); otherwise the forward adds one row-dot launch after the embeddings.  goal_feat must be
 * complete on the forward's stream (the cached goal embedding of the later steps of an episode).  Disarmed by that forward,
 * whatever it ran, or by (NULL, NULL). */
int var_set_reward_dot(var_ctx* ctx, const float* goal_feat, float* reward_out);

/* autograd backward of the encoder (loss.backward(), VAR/pretext_VAR.py:68) from the
 * gradients of the three embeddings; writes d(loss)/d(param) for all 213478
 * parameters into `grads` (overwrites; arena layout).  Any g_* may be NULL (= zeros). */
int var_arm_encoder_bwd(var_ctx* ctx, void* stream, const float* params,
                        const float* g_image_feat, const float* g_pos_feat, const float* g_neg_feat,
                        float* grads);

/* torch.nn.TripletMarginLoss(margin, p=2, eps=1e-6, reduction='mean')
 * (VAR/pretext_VAR.py:38,64) forward + backward in one launch.
 * loss_out[0] = sum_i hinge_i * inv_count;  g* = d(loss_out)/d(a|p|n).
 * inv_count = 1/B for the reference's mean; 1/B_global under data parallelism.
 * A row whose hinge argument d(a,p) - d(a,n) + margin is exactly 0 counts as inactive (zero gradients), like every
 * negative one.  ga, gp, gn may each be NULL (not written). */
int var_triplet_fwd_bwd(var_ctx* ctx, void* stream, const float* a, const float* p, const float* n,
                        int B, float margin, float inv_count,
                        float* loss_out, float* ga, float* gp, float* gn);

/* One fused training-step body: zero_grad -> model(image,pos,neg) -> triplet loss ->
 * backward (VAR/pretext_VAR.py:56-68), everything up to but excluding optimizer.step().
 * grads (arena) and loss_out[0] are overwritten.  feats_out: NULL, or 9*B floats = three (B,3) blocks
 * [image_feat | pos_feat | neg_feat]. */
int var_arm_loss_grad(var_ctx* ctx, void* stream, const float* params,
                      const void* image, int image_is_u8, long image_bstride,
                      const float* mfcc_pos, const float* mfcc_neg, int B, int H,
                      float margin, float inv_count,
                      float* grads, float* loss_out, float* feats_out);

/* The same with the data-loader work of dataset.py:64-89 / Envs/audioLoader.py:147-157 folded in:
 * the batch is gathered by index from a dataset resident in HBM and the MFCC front-end runs
 * inside the step (by default with the rest of the sound branch on the library's side stream; see var_set_streams).
 *   image        dataset images (N,C>=3,H,H) u8|f32; sample b uses row image_index[b] (NULL: row b)
 *   pcm          dataset clips, rows of pcm_stride int16 samples; clip_index (2B) = [pos | neg] rows
 *                (NULL: rows 0..2B-1); lens (2B) valid samples per clip, 0 = the "empty" class whose
 *                MFCC is all zeros (dataset.py:37-38) */
int var_arm_loss_grad_pcm(var_ctx* ctx, void* stream, const float* params,
                          const void* image, int image_is_u8, long image_bstride, const int* image_index,
                          const int16_t* pcm, int pcm_stride, const int* clip_index, const int* lens,
                          int B, int H, float margin, float inv_count,
                          float* grads, float* loss_out, float* feats_out);

/* var_arm_loss_grad with the image batch gathered by index (sample b = row image_index[b] of the HBM-resident
 * dataset, as in var_arm_loss_grad_pcm) and the MFCC features given.  The data-parallel replayed step uses it: the
 * front-end of step k+1 (var_mfcc) is then enqueued between the gradient all-reduce of step k and its optimiser
 * step, so that the collective's latency hides behind work that does not depend on the weights. */
int var_arm_loss_grad_gather(var_ctx* ctx, void* stream, const float* params,
                             const void* image, int image_is_u8, long image_bstride, const int* image_index,
                             const float* mfcc_pos, const float* mfcc_neg, int B, int H,
                             float margin, float inv_count,
                             float* grads, float* loss_out, float* feats_out);

/* torch.optim.Adam(lr, betas, eps, weight_decay) .step() (VAR/pretext_VAR.py:33-35,69)
 * on flat arenas; `step` is the 1-based step count.  When n == VAR_N_PARAMS and
 * params is the model arena the packed weight images are refreshed as well. */
int var_adam_step(var_ctx* ctx, void* stream, float* params, const float* grads, float* exp_avg,
                  float* exp_avg_sq, long n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int step);

/* The same step with the step count (incremented here) and the learning rate read from DEVICE
 * memory, so that the launch can be captured once into a HIP graph and replayed every step
 * (MultiStepLR then updates *lr_dev between replays). */
int var_adam_step_dev(var_ctx* ctx, void* stream, float* params, const float* grads, float* exp_avg,
                      float* exp_avg_sq, long n, const float* lr_dev, float beta1, float beta2, float eps,
                      float weight_decay, int* step_dev);

/* var_adam_step_dev plus the data-loader cursor of a graph-replayed epoch: index_table (n_rows x row_ints int32,
 * e.g. [image_index | clip_index | lens] per step, built once per epoch on the device -- the reference's
 * DataLoader(shuffle=True), VAR/pretext_VAR.py:26-31,55) is walked on the DEVICE: at the end of the step row
 * (*cursor_dev + 1) mod n_rows is copied into index_row (the buffer the captured var_arm_loss_grad_pcm reads) and
 * *cursor_dev is advanced, so a replay needs no host-side copy.  One kernel launch does the Adam update, the
 * re-pack of the weight images, the step count and the row fetch.  ahead != 0: index_row holds TWO rows,
 * [row cursor+1 | row cursor+2] -- the data-parallel pipeline computes the MFCC features of step k+1 before the
 * optimiser step of step k, so its front-end reads the second copy while the gradient pass reads the first. */
int var_adam_step_graph(var_ctx* ctx, void* stream, float* params, const float* grads, float* exp_avg,
                        float* exp_avg_sq, long n, const float* lr_dev, float beta1, float beta2, float eps,
                        float weight_decay, int* step_dev, const int* index_table, int row_ints, int n_rows,
                        int* cursor_dev, int* index_row, int ahead);

/* The PPO update's optimiser step over a table of tensors (models/ppo/algo/ppo.py:32,89-91):
 *     nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)      # norm type 2
 *     self.optimizer.step()                                  # optim.Adam(lr, eps): weight decay 0, no amsgrad, no maximize
 * `segs` is a HOST array of 1..256 segments {p, g, m, v, n}: n floats each of a parameter, its gradient, exp_avg and
 * exp_avg_sq.  It travels to the kernels by value (as var_move_seg), VAR_OPT_MAX_SEGS segments per launch, and is not read after
 * the call returns.  Launches: the sums of squares (every workgroup leaves the sum over its share of all gradients in a
 * context buffer: no floating-point atomics), then clip and Adam -- two for a table of up to VAR_OPT_MAX_SEGS segments,
 * 2 * ceil(n_seg / VAR_OPT_MAX_SEGS) beyond, all sums of squares before any Adam.  Every workgroup of the second kind folds the
 * sums in the same order, forms total_norm = sqrt(sum) and coef = min(max_norm / (total_norm + 1e-6), 1) as clip_grad_norm_
 * does (a NaN norm gives a NaN coef), and applies to g' = g * coef
 *     m' = m + (g' - m) (1 - beta1);  v' = v beta2 + (1 - beta2) g' g';  p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)
 * with bc1, bc2 = 1 - beta^step formed in double from the advanced *step_dev and from *lr_dev on the device, as
 * var_adam_step_dev.  *step_dev is advanced by one per call (by the first launch, which stream order puts behind the last
 * call's readers).  total_norm_out (device, may be NULL) receives the UNCLIPPED norm, which is what clip_grad_norm_ returns.
 * max_norm <= 0: no clip -- no sum-of-squares launch (one thread advances the step instead), coef = 1, total_norm_out is
 * not written.
 * The gradients are NOT modified: PyTorch scales them in place, and nothing in PPO.update reads them afterwards.
 * Which workgroup and thread takes which element depends on the element's number in the table's concatenation and on the
 * total length alone, so equal inputs give equal bits, and so do the same tensors cut into segments differently (one merged
 * segment or many small ones, one launch or several): p, m, v and total_norm alike.  Pointers need 4-byte alignment only:
 * four consecutive elements of one segment are one 16-byte access per array (dword-aligned), elements next to a segment's end
 * go one by one.  Non-finite gradients behave as in PyTorch: they go through to the parameters, there is no guard word --
 * look at total_norm_out.
 * Stream-ordered; never synchronises, allocates or reads back, so the call can be captured (the graph then holds the
 * table's addresses).  One call at a time per context: the sums live in the context.
 * VAR_ERR_ARG, nothing launched or written: n_seg outside 1..256; a NULL pointer in a segment, NULL lr_dev or step_dev;
 * n < 1; a pointer that is not 4-byte aligned; beta1 or beta2 outside [0, 1); eps < 0; NaN in max_norm, a beta or eps; any
 * two ranges of the table (p, g, m, v of all segments, and the three scalars) that overlap. */
#define VAR_OPT_MAX_SEGS 64
typedef struct var_opt_seg { float* p; const float* g; float* m; float* v; long n; } var_opt_seg;
int var_clip_adam_step(var_ctx* ctx, void* stream, const var_opt_seg* segs /* host */, int n_seg,
                       float max_norm /* <= 0: no clip */, const float* lr_dev, float beta1, float beta2, float eps,
                       int* step_dev, float* total_norm_out /* device, 1 float; may be NULL */);

/* Audio front-end: Envs/audioLoader.py:147-157 (torchaudio MFCC branch) + :241-252
 * (processSoundFeat).  pcm: rows of `pcm_stride` int16 samples; output clip i reads row
 * clip_index[i] (NULL: row i) and lens[i] valid samples (<= pcm_stride; 0 = "empty" class =>
 * zeros); out: (nclips, 1, out_frames, 40) f32, frames beyond 1 + len/160 are zero
 * (MFCC-domain padding), frames beyond out_frames are dropped.  A clip of 1..256 samples is outside the domain of
 * the reference (torch.stft's reflect padding needs more than n_fft / 2 samples): its 1 + len/160 rows are finite but
 * pinned by no reference, the rows behind them zero; lens[i] > pcm_stride reads as pcm_stride.  More than 2^23
 * output frames (nclips * out_frames) in one call are refused. */
int var_mfcc(var_ctx* ctx, void* stream, const int16_t* pcm, const int* lens, const int* clip_index,
             int nclips, int pcm_stride, int out_frames, float* out);

/* Clip cache of the front-end above, for a pool of clips that is read again and again (the reference's
 * VARFineTuneDataset computes each item's MFCC once, dataset.py:94-133).  The CALLER owns both buffers and fills them:
 *   cache_feats  f32 [rows][out_frames][40], device: row r = what var_mfcc(pcm, lens = cache_lens, clip_index = NULL, nclips =
 *                rows, out_frames) writes for it;
 *   cache_lens   int32 [rows], device: the length row r's features were computed for; negative = row r is not cached.
 * The library only remembers the pointers, between a bind and the next unbind (or bind): a binding is meant to be SCOPED --
 * bind, enqueue or capture, unbind -- and the buffers must stay alive and unchanged for as long as work enqueued (or a
 * graph captured) under the binding may run.  While it is in place, every 512/400/160 front-end launch of this context
 * (var_mfcc, var_mfcc_ex with those parameters, var_arm_loss_grad_pcm) whose pcm, pcm_stride and out_frames equal the bound
 * ones decides PER SLOT, on the device: slot i is SERVED -- out[i] = cache_feats[row], no transform, the clip's samples are
 * not read -- when row = clip_index ? clip_index[i] : i lies in [0, rows), lens[i] > 0 and lens[i] == cache_lens[row]; every
 * other slot (the empty class, another length, a row that is not cached) is computed as without a binding.  Frames are
 * computed independently of their neighbours, so a served slot holds the very bits a live one gets.  Launches with another
 * pcm pointer, stride or out_frames, var_mfcc_psf and var_mfcc_ex's other configurations ignore the binding.
 * var_arm_loss_grad_pcm under a binding reads served clips IN PLACE: its sound CNN, forward and backward, takes a served
 * slot's features from cache_feats[row] and an empty slot's (lens[i] <= 0) from nowhere, and the front-end neither copies nor
 * zeroes those slots of the library's feature buffer; live slots go through the buffer as before.  Same bits either way; bit 7
 * of var_set_streams keeps the copy.  LIFETIME: the pool, cache_feats, cache_lens, and the step's lens and clip_index must
 * stay unchanged from the enqueue of that forward until the last backward of it has run -- the fused step's own, and a later
 * var_arm_encoder_bwd of the same forward if one is made.  (VARTrainer complies: the captured step's index row is rewritten by
 * the optimiser launch, behind the join of both branches.)  var_mfcc and var_mfcc_ex hand features to the caller and always
 * copy.
 * VAR_ERR_ARG: a NULL pointer, rows, pcm_stride or out_frames < 1, rows * out_frames >= 2^31. */
int var_mfcc_cache_bind(var_ctx* ctx, const int16_t* pcm, int rows, int pcm_stride, int out_frames,
                        const int* cache_lens, const float* cache_feats);
int var_mfcc_cache_unbind(var_ctx* ctx);

/* The same front-end with the STFT parameters of the dataset a clip comes from (Envs/audioLoader.py:23-31, param_dict:
 * nFFT / int(windowLenTime * fs) / int(windowStepTime * fs)): 512 / 400 / 160 for GoogleCommand, FSC, ESC50, Spatial,
 * Synthetic -- var_mfcc's kernel -- and 1024 / 800 / 640 for NSynth and UrbanSound, or any power-of-two n_fft in
 * 64..2048 with win_length <= n_fft; T = 1 + len / hop_length frames.  The first call for a new configuration builds
 * its tables (it allocates: make it once outside graph capture). */
int var_mfcc_ex(var_ctx* ctx, void* stream, const int16_t* pcm, const int* lens, const int* clip_index,
                int nclips, int pcm_stride, int out_frames, int n_fft, int win_length, int hop_length, float* out);

/* iTHOR model ------------------------------------------------------------------------------
 * The second VARPretextNet of the reference (models/pretext/ai2thor_pretext_model.py:5-58, config 4 of
 * BASELINE.json): stride-1 3x3 convolutions with 2x2 max pools on the image, three wide stride-2 convolutions
 * and a bidirectional GRU(448 -> 512) on the (1,600,40) sound features, Linear heads, F.normalize.  Parameters
 * are its 36 state_dict() tensors back to back in registration order (imgBranch.{0,2,5,8,11,14}, rnn.*_l0,
 * rnn.*_l0_reverse, cnn.{0,2,4}, imgTriplet.{0,2}, soundTriplet.{0,2,4}), each in its PyTorch layout:
 * var_ithor_param_count() = 3849126 floats.  The entries mirror the Kuka ones above (same argument meaning);
 * image_raw is (B,1152), pos_raw (B,1024); img_hw is any side that ends in a 3x3 map (96, 84).
 * var_adam_step / var_triplet_fwd_bwd are shared with the Kuka model. */
int var_ithor_param_count(void);
int var_ithor_plan(var_ctx* ctx, int max_batch, int img_hw);
/* Operand precision of every product of the iTHOR model: 0 = fp32 (default; the parity path), 1 = bf16 operands
 * (round to nearest even) with fp32 accumulation on v_mfma_f32_32x32x16_bf16 -- BASELINE config 4's stated precision;
 * parameters, gradients, the optimiser state and every activation the model returns stay fp32.  The sound CNN's
 * intermediate maps then live as bf16 images only; 2 = as 1, and the fp32 copies of those maps (conv 1 / conv 2 outputs and
 * the gradient wrt conv 2's output: 1.3 GB of stores per step at batch 256 that nothing but var_debug_buffer reads) are
 * written too -- what the layer-wise parity tests use.  -1 = query.  Returns the previous setting (or a negative error
 * code); call after var_ithor_plan. */
int var_ithor_set_bf16(var_ctx* ctx, int on);
/* bf16 mode only: run the 73 time steps of each GRU pass as ONE persistent launch (1, the default) in which the workgroups
 * of a 64-clip slice hand the recurrent state to each other through memory, or as one launch per time step (0).  Both
 * give bit-identical results.  The persistent form needs its whole grid (32 workgroups per 64 clips) resident at once:
 * it is skipped by itself when the grid exceeds the device's CU count, and every wait in it is bounded -- if a wait
 * expires (e.g. another process holds part of the GPU) the launch ends and the step's embeddings / gradient are
 * overwritten with NaN rather than left partially updated.  The time-out word of the CURRENT step also guards the
 * optimiser: var_adam_step / var_adam_step_dev over this model's arena (n == var_ithor_param_count()) then leave
 * parameters, moments and step count untouched, so a transient time-out costs one step, not the run.  The next
 * var_ithor_* forward clears the current word by itself and files the event in two sticky words (count, last code).
 * var_ithor_gru_status copies the status (blocking): the current step's code (1 + t forward, 101 + t backward) if it
 * timed out, else 0x40000000 | code of the last earlier time-out, else 0.  The residency test uses the occupancy the
 * runtime grants the two sequence kernels (hipOccupancyMaxActiveBlocksPerMultiprocessor), not just the CU count.
 * -1 = query; returns the previous setting; setting a form (0 / 1) also clears every status word (after a
 * hipDeviceSynchronize-like wait on the null stream). */
int var_ithor_set_gru_sequence(var_ctx* ctx, int on);
int var_ithor_gru_status(var_ctx* ctx, unsigned* word);
/* Data parallelism: the time-out word above is per rank, but the poisoned gradient of the rank that timed out is summed into
 * every rank's buffer by the all-reduce.  var_ithor_guard_loss names a device float that var_adam_step / var_adam_step_dev over
 * this model's arena read at launch time as a second guard: not finite = leave parameters, moments and step count alone.
 * Point it at the loss slot that travels with the gradient through the all-reduce (the timed-out rank's loss is NaN, so the
 * sum is NaN on every rank) and all replicas skip the same step.  NULL removes the guard.  The pointer is read when an Adam
 * launch is enqueued (a captured launch keeps the one it was captured with). */
int var_ithor_guard_loss(var_ctx* ctx, const float* loss_dev);
int var_ithor_encoder_fwd(var_ctx* ctx, void* stream, const float* params,
                          const void* image, int image_is_u8, long image_bstride,
                          const float* snd_pos, const float* snd_neg, int B, int H,
                          float* image_feat, float* pos_feat, float* neg_feat,
                          float* image_raw, float* pos_raw, int save_for_bwd);
int var_ithor_saved_generation(var_ctx* ctx);     /* as var_saved_generation, for the iTHOR workspace */
int var_ithor_encoder_bwd(var_ctx* ctx, void* stream, const float* params,
                          const float* g_image_feat, const float* g_pos_feat, const float* g_neg_feat,
                          float* grads);
int var_ithor_loss_grad(var_ctx* ctx, void* stream, const float* params,
                        const void* image, int image_is_u8, long image_bstride,
                        const float* snd_pos, const float* snd_neg, int B, int H,
                        float margin, float inv_count,
                        float* grads, float* loss_out, float* feats_out);

/* In-batch-negatives contrastive head (BASELINE.json configs[2]; an EXTENSION without a reference counterpart --
 * the reference trains with the explicit-negative triplet loss above).  anchor (B,3) = the local image embeddings,
 * cand (M,3) = the candidate sound embeddings of the GLOBAL batch (every rank's [positives ; negatives],
 * var_allgather_emb), target[i] = column of sample i's positive.
 *   L = inv_count * sum_i [ logsumexp_j(-d_ij / tau) + d_{i,target[i]} / tau ],  d_ij = ||a_i - c_j + 1e-6||_2
 * loss_out[0] = this rank's share of L; g_anchor (B,3) = dL/da; g_cand (M,3) = the gradient wrt every candidate from
 * this rank's rows (sum over the ranks -- var_allreduce_grads on it -- and keep your own rows).  scratch: 2*B floats.
 * One wavefront per row / per candidate, wave-shuffle softmax, no atomics. */
int var_inbatch_loss_fwd_bwd(var_ctx* ctx, void* stream, const float* anchor, const float* cand, const int* target,
                             int B, int M, float tau, float inv_count, float* scratch, float* loss_out,
                             float* g_anchor, float* g_cand);

/* The class-aware forms of the head above (which ignores labels: with taskNum + 1 classes about a fifth of an anchor's other
 * candidates carry the anchor's own class and are pushed away as negatives; the triplet loss never draws such a negative,
 * dataset.py:70-78).  anchor_cls (B) = y_i, cand_cls (M) = z_j, int32 on the device; l_ij = -d_ij / tau, t(i) = target[i]:
 *   VAR_INBATCH_ALL             L_i = logsumexp_j l_ij - l_{i,t(i)}: var_inbatch_loss_fwd_bwd bit for bit; the class pointers
 *                               are not read and may be NULL.
 *   VAR_INBATCH_OTHER_CLASS     L_i = logsumexp_{j in N_i} l_ij - l_{i,t(i)},  N_i = { j : z_j != y_i } + { t(i) }: the other
 *                               candidates of the anchor's class take no part, in the sum or in any gradient.
 *   VAR_INBATCH_MULTI_POSITIVE  L_i = logsumexp_j l_ij - (1/|P_i|) sum_{p in P_i} l_ip,  P_i = { j : z_j = y_i } + { t(i) }
 *                               (the supervised-contrastive form with the positives outside the log).
 * loss_out[0] = inv_count * sum_i L_i; gradients and their use under data parallelism as above.  z_{t(i)} = y_i is not
 * required; target[i] in [0, M) is the caller's duty.  scratch: 3*B floats.  A mode whose masks select nothing (no class
 * shared) gives the bits of mode 0.  VAR_ERR_ARG, nothing written: what the entry above refuses, a mode outside 0..2, a NULL
 * class pointer in mode 1 or 2. */
enum { VAR_INBATCH_ALL = 0, VAR_INBATCH_OTHER_CLASS = 1, VAR_INBATCH_MULTI_POSITIVE = 2 };
int var_inbatch_loss_fwd_bwd_ex(var_ctx* ctx, void* stream, const float* anchor, const float* cand, const int* target,
                                const int* anchor_cls, const int* cand_cls, int B, int M, float tau, float inv_count,
                                int mode, float* scratch, float* loss_out, float* g_anchor, float* g_cand);

/* Collectives ----------------------------------------------------------------------------------
 * For hosts without torch.distributed: one RCCL communicator per context.  Rank 0 obtains a 128-byte unique id
 * (var_comm_unique_id), the host ships it to the other ranks over its own channel, every rank calls var_comm_init.
 * var_allreduce_grads: in-place sum over the ranks of the flat gradient arena (append the loss as one more float and
 * it travels in the same message) -- the ONE exchange of the data-parallel step, between var_*_loss_grad
 * (inv_count = 1/B_global) and var_adam_step.  var_allgather_emb: global[r*n_local ...] = rank r's `local`
 * (embeddings for an in-batch-negatives loss; BASELINE config 3's extension).  Stream-ordered like every other
 * entry.  librccl.so is opened on first use (dlopen), not at load time. */
int var_comm_unique_id(var_ctx* ctx, void* id128);
int var_comm_init(var_ctx* ctx, int rank, int nranks, const void* id128);
int var_comm_destroy(var_ctx* ctx);
int var_allreduce_grads(var_ctx* ctx, void* stream, float* flat_grad, long n);
int var_allgather_emb(var_ctx* ctx, void* stream, const float* local, float* global, long n_local);

/* RL actor-critic forward ---------------------------------------------------------------
 * Policy.act up to the sampling (models/ppo/model.py:57-69): armNet_VAR.forward (models/RL/arm_RL_model.py:99-134, the
 * 96x96 image branch, recurrent: one GRU(128 -> 512) step from rnn_hxs * masks, models/ppo/model.py:118-121) and the
 * mean layer of DiagGaussian (models/ppo/distributions.py:65-84).  Kuka configuration: representationDim 3,
 * robotStateDim 2, RLRecurrentInputSize 128, RLRecurrentSize 512, RLActionHiddenSize 128, actionDim 2
 * (fourInARow/config.py:67-106, kuka/env_config.py:37).  params = Policy.state_dict() back to back in registration
 * order (base.gru.*, base.imgCNN.{0,2,5,7,10,12,15,17}, base.motorMlp, cnnMlp, imgMotorMlp, imgMotorMlp2, soundMlp,
 * fusionMlp, mlp_all, actor, critic, critic_linear, dist.fc_mean, dist.logstd._bias): var_armnet_param_count() floats.
 *   image (B,3,96,96) u8 (divided by 255) or f32; image_feat (B,3), robot_pose (B,2), goal_sound_feat (B,3),
 *   rnn_hxs (B,512), masks (B,1)  ->  value (B,1), actor_features (B,128), action_mean (B,2, may be NULL),
 *   rnn_hxs_out (B,512).  Sampling / log-probabilities (a handful of flops) stay with the caller.
 * Kernel paths (same results within 2e-5): B <= 64 images run the convolutions on LDS-band kernels with the pools fused, the
 * filters re-packed inside the first launch of every call (parameters updated in place between two calls are picked up);
 * B <= 8 rows (the RL stage's envs) run the 22 Linear layers + GRU step as one persistent launch whose workgroups hand their
 * vectors over as (value, epoch) pairs -- it needs its 128 workgroups co-resident; if they are not, every wait times out
 * (bounded: a workgroup gives up all its later waits at once after its first expired one) and the outputs are NaN.  The
 * reference's Policy.act (models/ppo/model.py:57-69) has no failure mode, so this one is reported: var_armnet_status copies
 * (blocking) 1 if the most recent chain launch timed out, 0x40000001 if an earlier one did since the last
 * var_armnet_clear_status, else 0; a timed-out launch leaves nothing behind -- the next one is clean.  rnn_hxs_out must not
 * overlap rnn_hxs (VAR_ERR_ARG: the chain reads the old state from all workgroups of its GRU stage while one writes the new
 * one).  Captured into a HIP graph the call replays as 9 kernel nodes. */
int var_armnet_param_count(void);
int var_armnet_plan(var_ctx* ctx, int max_batch);
int var_armnet_forward(var_ctx* ctx, void* stream, const float* params, const void* image, int image_is_u8,
                       long image_bstride, const float* image_feat, const float* robot_pose,
                       const float* goal_sound_feat, const float* rnn_hxs, const float* masks, int B,
                       float* value, float* actor_features, float* action_mean, float* rnn_hxs_out);
int var_armnet_status(var_ctx* ctx, unsigned* word);
int var_armnet_clear_status(var_ctx* ctx);

/* iTHOR RL actor-critic forward -------------------------------------------------------------------------------
 * Policy.act up to the sampling (models/ppo/model.py:57-69) for base 'ai2thor_VAR' (Envs/ai2thor/config.py:71):
 * ai2thorNet_VAR.forward (models/RL/ai2thor_RL_model.py:87-121: the 96x96 image stack, the 9x9 occupancy branch, recurrent:
 * one GRU(128 -> 1024) step from rnn_hxs * masks) and the linear layer of Categorical (n_actions logits).  params =
 * Policy.state_dict() back to back in registration order (base.gru.*, base.imgCNN.{0,2,5,8,11,14},
 * base.occupancyCNNMLP.{0,2,5,7}, base.motorMlp, cnnMlp, imgMotorMlp, imgMotorMlp2, soundMlp, fusionMlp, mlp_all, actor,
 * critic, critic_linear, dist.linear): var_ithor_policy_param_count(n_actions) floats (5 475 081 at 8 actions; 1 <= n_actions
 * <= 16, else VAR_ERR_ARG).
 *   image (B,3,96,96) and occupancy (B,1,9,9, contiguous), each u8 (divided by 255) or f32 already divided; image_feat (B,3),
 *   goal_sound_feat (B,3), rnn_hxs (B,1024), masks (B,1)  ->  value (B,1), actor_features (B,128), logits (B,n_actions, may be
 *   NULL), rnn_hxs_out (B,1024).  Sampling / log-probabilities stay with the caller.
 * Kernel paths as var_armnet_forward's (same results within 2e-5): B <= 64 images on the LDS-band convolutions, B <= 8 rows
 * on the one-launch MLP chain, which reports time-outs through var_ithor_policy_status / var_ithor_policy_clear_status with
 * var_armnet_status's semantics.  rnn_hxs_out must not overlap rnn_hxs (VAR_ERR_ARG). */
int var_ithor_policy_param_count(int n_actions);
int var_ithor_policy_plan(var_ctx* ctx, int max_batch);
int var_ithor_policy_forward(var_ctx* ctx, void* stream, const float* params, int n_actions, const void* image, int image_is_u8,
                             long image_bstride, const void* occupancy, int occupancy_is_u8, const float* image_feat,
                             const float* goal_sound_feat, const float* rnn_hxs, const float* masks, int B,
                             float* value, float* actor_features, float* logits, float* rnn_hxs_out);
int var_ithor_policy_status(var_ctx* ctx, unsigned* word);
int var_ithor_policy_clear_status(var_ctx* ctx);

/* The acting forwards with bf16 operands ---------------------------------------------------------------------------------
 * var_armnet_forward_ex / var_ithor_policy_forward_ex take the argument lists above plus `flags`; the entries above are
 * _ex(..., 0) and keep their bits.
 *   flags bit 0   bf16 operands in every convolution of imgCNN (conv 1-8 of armNet_VAR, conv 1-6 of ai2thorNet_VAR), with the
 *       rounding points of var_convstack_fwd_ex's flags bit 0 (below), so that the rollout's old log-probabilities and the PPO
 *       update's evaluation come from one function: layer l computes relu(conv(bf16(x_l), bf16(w_l)) + b_l); x_1 is the float
 *       image exactly as the fp32 path forms it from bytes ((float)u8 / 255.f, or the float input), x_l the stored fp32 map
 *       below, pooled where a pool follows; rounding is to nearest even; products accumulate in fp32; bias and ReLU act in
 *       fp32; pools act on fp32 values; everything stored stays fp32, in the layouts and var_debug_buffer names of the fp32
 *       forward.  The iTHOR occupancy convolutions, the MLP chain and the per-layer MLP, the GRU step, the head and
 *       var_policy_dist stay fp32.  Kernels, up to 64 images: the 3x3 / stride 1 / pad 1 band layers behind conv 1 (conv 2-6 of
 *       armNet_VAR, conv 2-5 of ai2thorNet_VAR) run on csrc/c3f_bf16.h's band kernel -- the band rounded as it is written to LDS
 *       into a channel-innermost bf16 image, the filters packed as bf16 A fragments inside conv 1's launch,
 *       v_mfma_f32_16x16x32_bf16, the fp32 kernel's epilogue and fused pool; conv 1 and the small last layers (conv 7 / 8, iTHOR's
 *       conv 6) keep csrc/c3f.h's fp32 kernels and round both operands where they stage them -- a product of two bf16 values is
 *       exact in fp32, so that IS the definition above, summed in the fp32 forward's order.  Beyond 64 images every layer takes
 *       the gather-GEMM with its operands rounded on the way into v_mfma_f32_32x32x16_bf16.
 *   A plan (var_armnet_plan / var_ithor_policy_plan) serves both precisions; the filter tables are re-packed inside the first
 *   launch of every call in the call's precision.  Any other flag bit is refused: VAR_ERR_ARG, the entry's name first in the
 *   message, nothing launched or written. */
int var_armnet_forward_ex(var_ctx* ctx, void* stream, const float* params, const void* image, int image_is_u8,
                          long image_bstride, const float* image_feat, const float* robot_pose,
                          const float* goal_sound_feat, const float* rnn_hxs, const float* masks, int B,
                          float* value, float* actor_features, float* action_mean, float* rnn_hxs_out, int flags);
int var_ithor_policy_forward_ex(var_ctx* ctx, void* stream, const float* params, int n_actions, const void* image,
                                int image_is_u8, long image_bstride, const void* occupancy, int occupancy_is_u8,
                                const float* image_feat, const float* goal_sound_feat, const float* rnn_hxs, const float* masks,
                                int B, float* value, float* actor_features, float* logits, float* rnn_hxs_out, int flags);

/* The distribution tail of Policy.act -------------------------------------------------------------------------------
 * What follows the forward in models/ppo/model.py:59-69: the action (dist.sample() or dist.mode()) and dist.log_probs(action)
 * of DiagGaussian / Categorical (models/ppo/distributions.py:7-33, 60-84), ONE launch instead of about a dozen on (B,n)
 * tensors; the entropy act() computes and discards is not computed.  fp32 throughout.
 *   kind 0, DiagGaussian (1 <= n <= 4): head = action mean (B,n), logstd (n) (dist.logstd._bias); std = exp(logstd),
 *       action f32 (B,n) = mean + std * z, or mean itself when deterministic (FixedNormal.mode);
 *       logp (B,1) = sum_d( -(action - mean)^2 / (2 std^2) - logstd - 0.5 ln(2 pi) )  (torch.distributions.Normal.log_prob).
 *   kind 1, Categorical (1 <= n <= 16): head = logits (B,n), logstd ignored; p = softmax(logits) with the row maximum
 *       subtracted; action int64 (B,1) = the number of k in [0, n-1) with cdf_k <= u (inverse CDF: never above n - 1), or the
 *       FIRST index of the largest logit when deterministic (FixedCategorical.mode); logp (B,1) = log_softmax(logits)[action].
 * Noise.  noise_in given: the caller's values, z (B,n) for kind 0, u (B) for kind 1; rng_state is not touched.  noise_in NULL:
 * Philox4x32-10 with key {rng_state[0], rng_state[1]} and counter {rng_state[2], rng_state[3], row, 0} -> words x0..x3 per row;
 * u(x) = ((x >> 8) + 0.5) * 2^-24 evaluated in fp32 (exact below one half, round-to-even above: (0, 1], the largest word gives
 * 1.0f); kind 1 takes u(x0); kind 0 takes Box-Muller pairs z0 = sqrt(-2 ln u(x0)) cos(2 pi u(x1)), z1 = ... sin, and z2, z3 from
 * (x2, x3) the same way.  The 64-bit step {rng_state[2] low, rng_state[3] high} advances by one per launch, on the device (the
 * last workgroup to arrive stores it; nothing waits for another workgroup): a captured graph draws fresh noise on every replay
 * with no host write.  Launches that share one rng_state, and launches of more than one workgroup (B > 256, or a carry
 * beyond 8192 floats) on one context, must be stream-ordered with each other (one arrival counter per context).  noise_out (same shape as noise_in, may be NULL) receives
 * the noise used.  A deterministic launch reads no noise, writes no noise_out and leaves the step alone.
 * Carry.  hxs_src given: the same launch also copies B * hidden floats to hxs_dst -- after var_*_forward wrote rnn_hxs_out, this
 * puts it where the next forward reads rnn_hxs, so one static graph feeds its own next step (the forwards refuse in-place).
 * VAR_ERR_ARG: B < 1, n out of range, kind not 0 / 1, NULL head / action / logp (/ logstd for kind 0), sampling with neither
 * noise_in nor rng_state, hxs_src with NULL hxs_dst or hidden < 1, hxs_dst overlapping hxs_src.  A failed call launches
 * nothing.  B is not bounded (rows are spread over workgroups of 256). */
int var_policy_dist(var_ctx* ctx, void* stream, int kind /*0 DiagGaussian, 1 Categorical*/,
                    const float* head /* (B,n): action mean | logits */, const float* logstd /* (n) | NULL */,
                    int n, int B, int deterministic,
                    const float* noise_in /* NULL = built-in generator */, unsigned* rng_state /* 4 words, device */,
                    float* noise_out /* may be NULL */, void* action /* f32 (B,n) | int64 (B,1) */, float* logp /* (B,1) */,
                    const float* hxs_src, float* hxs_dst, int hidden /* hxs_src NULL = no carry */);

/* The PPO rollout around the networks: storage, returns, loss head --------------------------------------------------------
 * What models/ppo/storage.py and the loss lines of models/ppo/algo/ppo.py:38-87 do with dozens to hundreds of launches on
 * (N,1) / (T*N,1) tensors, as three entries of ONE launch each.  The networks' evaluation forward and backward stay with the
 * caller (PyTorch autograd).  fp32; no entry waits for another workgroup, allocates or synchronises.
 *
 * var_rollout_move: one strided row copy.  `segs` is a HOST array of 1..VAR_MOVE_MAX_SEGS segments (it travels to the kernel
 * by value: nothing is read from it after the call returns).  For every segment, every t < n_t and every j < n_env,
 *     e = ind ? ind[j] : j;   row_bytes bytes go from  src + t * src_t_stride + e * src_env_stride
 *                                               to    dst + t * dst_t_stride + j * dst_env_stride      (strides in bytes).
 * ind: device int32 (n_env) or NULL; n_src_env: the envs the source holds -- a row whose index lies outside [0, n_src_env) is
 * left unwritten (the list lives on the device: the host cannot refuse it).  dtype-blind: 16-byte pieces when both ends,
 * row_bytes and all four strides of a segment are multiples of 16, 4-byte words when of 4, bytes otherwise.  Uses:
 *   RolloutStorage.insert (storage.py:61-77): n_t = 1, destinations slot step + 1 of obs / hidden states / masks / bad_masks and
 *       slot step of actions / log-probs / value_preds / rewards;
 *   after_update (:79-87): slot T -> slot 0;
 *   one minibatch of recurrent_generator (:173-245): n_t = T, ind = the minibatch's envs, dst_t_stride = Nb * row_bytes,
 *       dst_env_stride = row_bytes: output row t * Nb + j, _flatten_helper's (T, Nb) -> T * Nb; the hidden state is a
 *       further segment with n_t = 1 reading slot 0.
 * VAR_ERR_ARG: no / too many segments, NULL end, row_bytes / n_t / n_env / n_src_env < 1, a negative stride, n_env > n_src_env
 * without ind, destination rows of a segment that overlap each other (dst_env_stride < row_bytes, or dst_t_stride smaller
 * than a step's rows), a destination range -- first to last byte a segment may touch -- that overlaps any segment's source
 * range or another segment's destination range, more than 2^31 - 1 workgroups.  A failed call launches nothing.
 *
 * var_rollout_returns: compute_returns (storage.py:89-128) in all four modes and the advantage normalisation of
 * ppo.py:39-41, one workgroup.  rewards (T,N,1), value_preds / masks / bad_masks / returns (T+1,N,1), next_value (N,1),
 * advantages (T,N,1) or NULL.  bad_masks may be NULL without use_proper_time_limits.  GAE stores value_preds[T] = next_value,
 * the other mode returns[T] = next_value, as the reference.  With g = (float)gamma, gl = (float)(gamma * gae_lambda) (product
 * in double), per env, t = T-1 .. 0, each operation rounded to fp32 in this grouping (bit-equal to the reference on the CPU):
 *   GAE:          d = (r[t] + (g * v[t+1]) * m[t+1]) - v[t];  a = d + (gl * m[t+1]) * a;  proper: a = a * bm[t+1];  ret[t] = a + v[t]
 *   else, proper: ret[t] = ((ret[t+1] * g) * m[t+1] + r[t]) * bm[t+1] + (1 - bm[t+1]) * v[t]
 *   else:         ret[t] = (ret[t+1] * g) * m[t+1] + r[t]
 * advantages = (A - mean(A)) / (std(A) + 1e-5), A = ret[:T] - v[:T], std unbiased (T*N - 1), two passes (mean, then squared
 * deviations), summed in a fixed order: equal inputs give equal bits.  Envs beyond the workgroup's 256 threads are looped.
 * VAR_ERR_ARG: T or N < 1, a NULL pointer, advantages with T * N < 2 (no standard deviation), an output overlapping an input
 * or the other output.  A failed call launches nothing.
 *
 * var_ppo_head: the loss of ppo.py:66-87 for one minibatch of M rows and its gradients.  kind / n / head / logstd as
 * var_policy_dist; value, old_logp, adv, returns, value_preds (M,1); action f32 (M,n) | int64 (M,1) (a Categorical action
 * outside [0, n) gives NaN losses, never a read outside the row).  out[4] = {value_loss, action_loss, dist_entropy, total},
 * total = value_loss * value_coef + action_loss - dist_entropy * entropy_coef; g_head (M,n), g_value (M,1), g_logstd (n, kind 0;
 * may be NULL for kind 1) = d total / d head, value, logstd.  value_preds may be NULL without use_clipped_value_loss.
 * logp (M,1), may be NULL: the log-probabilities of `action` the ratio was taken from.
 *   logp: Gaussian sum_d( -(a - mu)^2 / (2 sigma^2) - logstd - 0.5 ln 2 pi ), Categorical log_softmax(head)[a];
 *   ratio = exp(logp - old_logp); action_loss = -mean(min(ratio * adv, clamp(ratio, 1 - clip, 1 + clip) * adv));
 *   value_loss = 0.5 mean(max((v - ret)^2, (vpc - ret)^2)), vpc = vp + clamp(v - vp, -clip, clip), or 0.5 mean((ret - v)^2);
 *   dist_entropy = dist.entropy().mean() (models/ppo/model.py:80): Gaussian, over M * n elements of 0.5 + 0.5 ln 2 pi +
 *   logstd_d; Categorical, over M rows of -sum_k p_k ln p_k.
 * Gradients at the kinks are autograd's:
 *   d action_loss / d logp = -adv * ratio / M where ratio * adv <= clamp(ratio) * adv, 0 elsewhere (torch.min splits a tie in
 *       halves and clamp's mask includes its ends: a tie is inside the clip range, where the halves add up, or has adv = 0);
 *   clipped value loss, l1 = (v - ret)^2, l2 = (vpc - ret)^2: weights (1,0) / (0,1) / (1/2,1/2) for l1 > / < / = l2, the l2
 *       branch passing only where |v - vp| <= clip:  d value_loss / d v = (w1 (v - ret) + w2 [|v - vp| <= clip] (vpc - ret)) / M;
 *   d logp / d l_k = [k = a] - p_k;  d logp / d mu_d = (a - mu) / sigma^2;  d logp / d logstd_d = (a - mu)^2 / sigma^2 - 1;
 *   d H_row / d l_k = -p_k (ln p_k + H_row);  d dist_entropy / d logstd_d = 1 / n.
 * The sums over rows (the three losses, g_logstd): rows are spread over at most 256 workgroups, each leaves partial sums in the
 * context, the last one to arrive folds them in a fixed order -- equal inputs give equal bits, nothing waits, M is not bounded.
 * Launches of more than one workgroup (M > 256) on one context must be stream-ordered with each other.
 * VAR_ERR_ARG: kind not 0 / 1, M < 1, n out of range, clip < 0 or NaN, a NULL pointer other than those named above.  A failed
 * call launches nothing. */
#define VAR_MOVE_MAX_SEGS 16
typedef struct var_move_seg {
    const void* src;
    void* dst;
    long row_bytes, n_t;
    long src_t_stride, dst_t_stride, src_env_stride, dst_env_stride;
} var_move_seg;
int var_rollout_move(var_ctx* ctx, void* stream, const var_move_seg* segs /* host */, int n_seg,
                     const int* ind /* device (n_env) | NULL */, int n_env, int n_src_env);
int var_rollout_returns(var_ctx* ctx, void* stream, const float* rewards, float* value_preds, const float* masks,
                        const float* bad_masks, const float* next_value, int T, int N, int use_gae, double gamma,
                        double gae_lambda, int use_proper_time_limits, float* returns, float* advantages /* may be NULL */);
int var_ppo_head(var_ctx* ctx, void* stream, int kind /*0 DiagGaussian, 1 Categorical*/, const float* head, const float* logstd,
                 const float* value, const void* action, const float* old_logp, const float* adv, const float* returns,
                 const float* value_preds, int n, long M, float clip, float value_coef, float entropy_coef,
                 int use_clipped_value_loss, float* out /* 4 */, float* g_head, float* g_value, float* g_logstd,
                 float* logp /* (M,1), may be NULL */);

/* The env wrapper's step on the device: reward, normaliser, insert ----------------------------------------------------------
 * What VecPretextNormalize.step_wait and calcReward do on the host between the simulator's return and the next act
 * (Envs/vec_env/vec_pretext_normalize.py:47-61, 96-101) and what RL.py:171-185 does with the result, as two entries of ONE
 * launch each whose arguments do not change from step to step: a captured graph replays them (csrc/env_step.hip).  Neither
 * entry waits for another workgroup, allocates or synchronises; there is no time-out and no status word.
 *
 * var_reward_norm_step: one workgroup, float64, each operation rounded once in the reference's grouping.  Inputs, device:
 * dot (N) f32 or NULL (= 0): embReward -- <image_feat, goal_sound_feat>, or with config.RLRewardSoundSound on the fp32 sum
 * <image_feat, goal_sound_feat> + <current_sound_feat, goal_sound_feat> that var_reward_dots / var_ithor_reward_step_ex leave
 * (the second term is part of `dot`: this entry is the same in both modes); env_reward (N) f64; done (N) u8; bad (N) u8 or NULL (no
 * 'bad_transition').  normalise = 0 is the wrapper built with ret=False.  State, device float64: ret (N), rms[3] = {mean, var,
 * count} of running_mean_std.py:4-35 (a fresh one is {0, 1, 1e-4}), episode (3N) = the running sum of the un-normalised step
 * reward, the sum of the last finished episode, the number of finished episodes per env (RL.py:171-176: the host reads it when it
 * logs), slot int32[2].  Outputs: reward, masks, bad_masks (N,1) f32, orig_reward (N) f64 (origStepReward, :53).  Per env i:
 *     rews = (double)dot[i] + env_reward[i]                                     (calcReward, :96-101: embReward + envReward)
 *     ret[i] = ret[i] * gamma + rews                                                                                      (:55)
 *     normalise: bm = mean_i ret, bv = mean_i (ret - bm) * (ret - bm); delta = bm - mean; total = count + N;
 *         m2 = (var * count + bv * N) + (((delta * delta) * count) * N) / total;
 *         mean = mean + (delta * N) / total; var = m2 / total; count = total                (running_mean_std.py:22-32)
 *         rews = clip(rews / sqrt(var + epsilon), -cliprew, cliprew)                              (:58; a NaN stays a NaN)
 *     reward[i] = (float)rews;  masks[i] = done[i] ? 0 : 1;  bad_masks[i] = bad && bad[i] ? 0 : 1       (RL.py:179-183)
 *     ret[i] = 0 where done[i]                                                                                            (:59)
 *     episode: run = episode[i] + (un-normalised rews); where done[i]: episode[N+i] = run, episode[2N+i] += 1, run = 0;
 *         episode[i] = run
 * The two sums over the envs are taken by one thread in numpy's order (np.add.reduce of a contiguous float64 vector of at
 * most 128 elements): N < 8 left to right; else eight running sums over blocks of eight, folded ((r0+r1)+(r2+r3))+((r4+r5)+
 * (r6+r7)), then the remaining N % 8 elements one by one -- the state equals the reference's numpy bit for bit.
 * slot: the kernel stores slot[1] = slot[0], then slot[0] = (slot[0] + 1) % num_steps: slot[1] is the rollout step this env
 * step's insert writes to, carried on the device so that the launch after it (var_rollout_move_at, given &slot[1]) needs no
 * host-computed address.
 * VAR_ERR_ARG: N < 1 or N > 128 (numpy's pairwise recursion starts there), num_steps < 1, a NULL pointer other than dot / bad,
 * an output or state range overlapping an input or another output.  A failed call launches nothing.
 *
 * var_rollout_move_at: var_rollout_move (same piece widths, same kernel body) without an index list, n_src_env = n_env, whose
 * destinations a device word selects: `segs` is a HOST array of 1..VAR_MOVE_MAX_SEGS entries (it travels by value), `slot` a
 * DEVICE pointer of which the kernel reads slot[0].  Segment k goes to seg.dst + (slot[0] + slot_add) * dst_slot_stride
 * (bytes), and is left unwritten when slot[0] + slot_add lies outside [0, n_slots) (the word lives on the device: the host
 * cannot refuse it).  dst_slot_stride = 0 makes the segment a plain copy: the word is not consulted and n_slots must be 1.
 * RolloutStorage.insert (storage.py:61-77) is slot_add = 1, n_slots = T + 1 for obs, hidden states, masks, bad_masks and slot_add =
 * 0, n_slots = T for actions, log-probs, value_preds, rewards, each seg.dst the store's slot 0 and dst_slot_stride one slot.
 * The piece width also has to divide dst_slot_stride.
 * VAR_ERR_ARG: everything var_rollout_move refuses of a segment; slot NULL, n_env < 1, dst_slot_stride < 0, n_slots < 1,
 * 0 < dst_slot_stride < one slot's rows; the overlap checks run over a segment's WHOLE slot range (first byte of slot 0 to last
 * byte of slot n_slots - 1) against every source range, every other destination range and the slot word.  A failed call
 * launches nothing. */
typedef struct var_move_at_seg {
    var_move_seg seg;
    long dst_slot_stride;
    int slot_add, n_slots;
} var_move_at_seg;
int var_reward_norm_step(var_ctx* ctx, void* stream, const float* dot /* (N) | NULL */, const double* env_reward,
                         const unsigned char* done, const unsigned char* bad /* (N) | NULL */, int N, double gamma,
                         double cliprew, double epsilon, int normalise, int num_steps, double* ret, double* rms /* 3 */,
                         double* episode /* 3N */, int* slot /* 2 */, float* reward, float* masks, float* bad_masks,
                         double* orig_reward);
int var_rollout_move_at(var_ctx* ctx, void* stream, const var_move_at_seg* segs /* host */, int n_seg,
                        const int* slot /* device */, int n_env);

/* A PPO minibatch step without the host: the head's Linear fused with the loss, a gather behind a cursor ----------------------
 * The two entries that let one captured sequence serve every minibatch of an update (csrc/ppo_step.hip).  Neither waits for
 * another workgroup, allocates or synchronises; neither uses a floating-point atomic.
 *
 * var_ppo_head_linear: dist.fc_mean / dist.linear (models/ppo/distributions.py) and var_ppo_head in one call of two launches.
 *   head (M,n) = features (M,128) . W^T + b, W (n,128) and b (n) in nn.Linear's layout; head is an output;
 *   out[4], g_value (M,1), g_logstd (n, kind 0): var_ppo_head's, computed on that head by var_ppo_head's own device code
 *       (csrc/ppo_row.h) in var_ppo_head's row -> thread -> workgroup layout: fed the returned head, var_ppo_head gives the
 *       same bits.  kind / n / the loss's inputs, formulas and kinks: see var_ppo_head;
 *   g_features (M,128) = g_head . W,  g_W (n,128) = g_head^T . features,  g_b (n) = sum over the rows of g_head, g_head being
 *       var_ppo_head's d total / d head (it is not written out).
 * Summation orders depend on (M, n) only, so equal inputs give equal bits: a head value is 8 partial dot products (lane p of
 * the row takes the 16-byte pieces p, p + 8, p + 16, p + 24, left to right) joined by a butterfly, plus b; a g_features value
 * runs over k = 0 .. n-1; g_W / g_b are summed per workgroup (rows grid-strided in rounds of 256 over at most 256 workgroups;
 * inside one, eight row slices r % 8, each in row order, added in index order) and the workgroups' partials are added in index
 * order by the second launch, which also folds the loss sums as var_ppo_head does.  The partials live in `workspace`:
 * var_ppo_head_linear_workspace_bytes(kind, n, M) bytes (VAR_ERR_ARG for a refused shape), 16-byte aligned, contents
 * irrelevant before and after.  M is not bounded.  Concurrent calls need distinct workspaces, nothing else.
 * stats / cursor (device, both or neither): stats holds n_stats_rows rows of {value_loss, action_loss, dist_entropy}, cursor is
 * int32[2].  The launch that writes out[4] then also writes the three losses to stats row cursor[1] -- a row index outside
 * [0, n_stats_rows) leaves stats unwritten (the word lives on the device: the host cannot refuse it) -- and then adds n_env to
 * cursor[0] and 1 to cursor[1]: cursor[0] is what var_rollout_move_cursor reads, and stream order puts this behind the gather
 * that read it.
 * VAR_ERR_ARG: everything var_ppo_head refuses; NULL features / W / b / head / g_features / g_W / g_b / workspace; a workspace
 * shorter than the query's bytes or not 16-byte aligned; features or g_features not 16-byte aligned (W may lie at any word); one of stats / cursor
 * without the other, n_stats_rows < 1 or n_env < 0 with them; an output (head, out, g_features, g_W, g_b, g_value, g_logstd,
 * workspace, stats, cursor) overlapping an input or another output.  A failed call launches nothing.
 *
 * var_rollout_move_cursor: var_rollout_move (same piece widths, same kernel body, same refusals) whose index list is
 * ind_base + cursor[0]: ind_base a DEVICE int32 list of n_ind entries, cursor a DEVICE pointer of which the kernel reads
 * cursor[0].  When cursor[0] < 0 or cursor[0] + n_env > n_ind nothing is written (the word lives on the device: the host
 * cannot refuse it).  With all minibatches' env lists of an update behind ind_base and var_ppo_head_linear advancing the
 * cursor, one captured launch gathers every minibatch.
 * VAR_ERR_ARG: everything var_rollout_move refuses; ind_base or cursor NULL, n_ind < 1, n_env > n_ind; a destination range that
 * holds the cursor word or overlaps the index list.  A failed call launches nothing. */
long var_ppo_head_linear_workspace_bytes(int kind, int n, long M);
int var_ppo_head_linear(var_ctx* ctx, void* stream, int kind /*0 DiagGaussian, 1 Categorical*/, const float* features /* (M,128) */,
                        const float* W /* (n,128) */, const float* b /* (n) */, const float* logstd, const float* value,
                        const void* action, const float* old_logp, const float* adv, const float* returns,
                        const float* value_preds, int n, long M, float clip, float value_coef, float entropy_coef,
                        int use_clipped_value_loss, float* head /* (M,n) */, float* out /* 4 */, float* g_features /* (M,128) */,
                        float* g_W /* (n,128) */, float* g_b /* (n) */, float* g_value, float* g_logstd, void* workspace,
                        long workspace_bytes, float* stats /* (n_stats_rows,3) | NULL */, int n_stats_rows,
                        int* cursor /* 2, device | NULL */, int n_env);
int var_rollout_move_cursor(var_ctx* ctx, void* stream, const var_move_seg* segs /* host */, int n_seg,
                            const int* ind_base /* device (n_ind) */, int n_ind, const int* cursor /* device */, int n_env,
                            int n_src_env);

/* The PPO update's recurrent sequence, forward and backward --------------------------------------------------------------
 * NNBase._forward_gru (models/ppo/model.py:116-171) of a one-layer, one-direction nn.GRU with biases, as PPO.update
 * (models/ppo/algo/ppo.py:55-58 -> Policy.evaluate_actions, model.py:75-83) runs it on every minibatch: x (T*N, I), hxs (N, H),
 * masks (T*N, 1), w_ih (3H, I), w_hh (3H, H), b_ih (3H), b_hh (3H) in nn.GRU's layout and gate order r, z, n.  For t = 0..T-1,
 * h_{-1} = hxs:
 *     h' = h_{t-1} * m_t (row-wise);  gi = W_ih x_t + b_ih;  gh = W_hh h' + b_hh
 *     r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r * gh_n), h_t = (1 - z) * n + z * h'
 * out (T*N, H) = every h_t, h_T (N, H) = h_{T-1}.  For 0/1 masks this IS the reference's segmented form (model.py:132-166: it
 * multiplies all rows by masks[t] at every step where some row is 0, and at the other steps every mask is 1.0) without the
 * device-to-host read of the zero steps (model.py:134-138); T = 1 is its single-step branch (model.py:117-120).  Other mask
 * values are multiplied in as they are, which the reference does not do.  fp32.  Step t's result does not depend on T: T
 * chained one-step calls fed with their own h_T give the bits of one T-step call.
 *   var_gru_seq_workspace_bytes  bytes of `workspace` either direction needs at this shape (VAR_ERR_ARG for a refused shape).
 *   var_gru_seq_fwd  1 + T launches (input projection, one per step).  saved: 5*T*N*H floats (r | z | n | gh_n | h', each
 *       (T*N, H)) for the backward, or NULL when nobody differentiates.  The workspace holds gi.
 *   var_gru_seq_bwd  (what autograd replays for model.py:116-171) given d_out (T*N, H) and d_hT (N, H) or NULL: d_x (T*N, I),
 *       d_hxs (N, H: what flows past m_0), d_w_ih, d_w_hh, d_b_ih, d_b_hh; masks carry no gradient.  x, masks, w_ih, w_hh as
 *       in the forward whose `saved` is passed.  One launch transposes w_hh into the workspace (per call: an optimiser moves the
 *       weights between two minibatches, nothing packed is kept), T + 1 step launches walk t downwards, then the batched
 *       products (split-K slabs in the workspace, added in slab order) and the bias column sums: no atomics, equal inputs give
 *       equal bits.  The gradients are stored, not accumulated.
 * Both are stream-ordered on `stream`, never synchronise, never allocate: every buffer is the caller's.  VAR_ERR_ARG, with a
 * message and nothing launched: H not a multiple of 64 or above 1024, I outside 1..1024, N outside 1..64, T < 1 (or T*N*3H
 * above 2^30), a workspace smaller than var_gru_seq_workspace_bytes, out overlapping x or hxs (h_T, saved and the workspace
 * may not overlap out or hxs either), a NULL pointer other than saved / d_hT, hxs / w_hh / out / saved / workspace not
 * 16-byte aligned.  No kernel waits for another workgroup: there is no time-out and no status word. */
long var_gru_seq_workspace_bytes(int T, int N, int I, int H);
int var_gru_seq_fwd(var_ctx* ctx, void* stream, const float* x, const float* hxs, const float* masks, const float* w_ih,
                    const float* w_hh, const float* b_ih, const float* b_hh, int T, int N, int I, int H, float* out,
                    float* h_T, float* saved /* may be NULL */, void* workspace, long workspace_bytes);
int var_gru_seq_bwd(var_ctx* ctx, void* stream, const float* x, const float* masks, const float* w_ih, const float* w_hh,
                    const float* saved, const float* d_out, const float* d_hT /* may be NULL */, int T, int N, int I, int H,
                    float* d_x, float* d_hxs, float* d_w_ih, float* d_w_hh, float* d_b_ih, float* d_b_hh, void* workspace,
                    long workspace_bytes);

/* The PPO update's MLP trunk, forward and backward -------------------------------------------------------------------------
 * Everything between imgCNN's flattened output and the distribution head of armNet_VAR (kind 0, models/RL/arm_RL_model.py:
 * 102-134) and ai2thorNet_VAR (kind 1, models/RL/ai2thor_RL_model.py:85-115), as PPO.update evaluates it on a minibatch of
 * M = T*N rows ordered (t, n).  Inputs: feat (M, 1152), motor_in (M, 5 | 3: kind 0's is cat(image_feat, robot_pose)), sound_in
 * (M, 3), occ (M, 288: occupancyCNNMLP's flattened convolution output, kind 1 only), hxs (N, H), masks (M, 1).  With every
 * named layer a Linear + ReLU:
 *     flat = cnnMlp(feat)   motor = motorMlp(motor_in)   sound = soundMlp(sound_in)   occv = occupancyCNNMLP[5..8](occ)
 *     x = imgMotorMlp((flat + motor) [+ occv])           g, h_T = the masked GRU above (x, hxs, masks), unchanged
 *     rnn = imgMotorMlp2(g)   fusion = fusionMlp(sound + flat)   y = mlp_all(fusion + rnn)
 *     value = critic_linear(critic(y)) (no ReLU on critic_linear)   actor_features = actor(y)
 * kind 0: H 512, motorMlp 5-256-512-256, imgMotorMlp 256-256-128 (20 layers); kind 1: H 1024, motorMlp 3-64-256, imgMotorMlp
 * 256-64-128, the occupancy branch (21 layers).  T = 1 is the single-step branch.  fp32; the ReLU gradient is autograd's
 * (zero where the output is zero).
 *   var_trunk_n_params / _param_floats / _grad_offset   the published parameter order: the four GRU tensors (weight_ih_l0,
 *       weight_hh_l0, bias_ih_l0, bias_hh_l0), then weight and bias of every trunk layer in the base's state_dict order
 *       (kind 1: occupancyCNNMLP.5, .7 first; then motorMlp, cnnMlp, imgMotorMlp, imgMotorMlp2, soundMlp, fusionMlp, mlp_all,
 *       actor, critic, critic_linear).  Gradient i lies at float offset var_trunk_grad_offset(kind, i) of the one flat d_params
 *       buffer, whose length is var_trunk_grad_offset(kind, n_params).  var_trunk_n_layers: (n_params - 4) / 2.
 *   var_trunk_saved_floats / _saved_offset   `saved` holds every layer's activation (M, out) in layer order (i < n_layers), then
 *       the GRU's output g (M, H) (i = n_layers), then var_gru_seq_fwd's own 5*M*H (i = n_layers + 1).
 *   var_trunk_fwd   `params`: a HOST array of n_params device pointers in the published order.  11 stage launches (layers of
 *       one dependency depth share a launch; the residual sums are added on load) + the GRU's 1 + T.  saved may be NULL (a
 *       forward nobody differentiates: the activations then live in the workspace).
 *   var_trunk_bwd   given d_value (M, 1), d_actor_features (M, 128), d_hT (N, H), each or all NULL (= zero): d_feat (M, 1152),
 *       d_occ (M, 288; kind 1), d_hxs (N, H) and every parameter's gradient in d_params; motor_in, sound_in and masks carry no
 *       gradient.  11 stage launches, each computing dX, dW and db of its layers with the ReLU gate formed on load, +
 *       var_gru_seq_bwd's.  Stored, not accumulated.  No atomics: equal inputs give equal bits.
 * Stream-ordered, never synchronise, never allocate.  VAR_ERR_ARG, with a message and nothing launched: a NULL pointer other than
 * those named, kind not 0 / 1, N outside 1..64, T < 1, T*N above 16384 rows, occ (d_occ) missing for kind 1, a workspace smaller
 * than var_trunk_workspace_bytes, an output overlapping an input or another output, hxs / saved / workspace not 16-byte aligned. */
int var_trunk_n_layers(int kind);
int var_trunk_n_params(int kind);
long var_trunk_param_floats(int kind, int i);
long var_trunk_grad_offset(int kind, int i);
long var_trunk_saved_offset(int kind, int T, int N, int i);
long var_trunk_saved_floats(int kind, int T, int N);
long var_trunk_workspace_bytes(int kind, int T, int N);
int var_trunk_fwd(var_ctx* ctx, void* stream, int kind, const float* const* params, const float* feat,
                  const float* occ /* kind 1 */, const float* motor_in, const float* sound_in, const float* hxs, const float* masks,
                  int T, int N, float* value, float* actor_features, float* h_T, float* saved /* may be NULL */, void* workspace,
                  long workspace_bytes);
int var_trunk_bwd(var_ctx* ctx, void* stream, int kind, const float* const* params, const float* feat,
                  const float* occ /* kind 1 */, const float* motor_in, const float* sound_in, const float* masks, int T, int N,
                  const float* saved, const float* d_value, const float* d_actor_features, const float* d_hT /* each may be NULL */,
                  float* d_feat, float* d_occ /* kind 1 */, float* d_hxs, float* d_params, void* workspace, long workspace_bytes);

/* The actor-critics' convolution stacks, forward and backward --------------------------------------------------------------
 * What PPO.update evaluates in front of the trunk above, on a minibatch of B = T*N observations.  Every convolution is 3 x 3
 * and followed by ReLU; "+pool" is MaxPool2d(2, 2); the output is the last map flattened as NCHW (Flatten()):
 *   kind 0  armNet_VAR.imgCNN, the 96 x 96 branch of buildCNN (models/RL/arm_RL_model.py:22-34): 3->32, 32->32 +pool, 32->64,
 *           64->64 +pool, 64->128, 128->128 +pool (stride 1, padding 1), 128->256 (stride 2, padding 0), 256->128 (stride 1,
 *           padding 0): image (B, 3, 96, 96) -> feat (B, 1152).  The other branch of buildCNN (7 x 7 filter, 120 x 160) has no
 *           kind: it is not implemented.
 *   kind 1  ai2thorNet_VAR.imgCNN (models/RL/ai2thor_RL_model.py:16-25): 3->32, 32->32 +pool, 32->64 +pool, 64->64 +pool,
 *           64->128 +pool (stride 1, padding 1), 128->128 (stride 2, padding 1): image (B, 3, 96, 96) -> feat (B, 1152).
 *   kind 2  the two convolutions of occupancyCNNMLP (ai2thor_RL_model.py:34-35): 1->64, 64->32 (stride 2, padding 1):
 *           image (B, 1, 9, 9) -> feat (B, 288), var_trunk_fwd's `occ`.
 * fp32.  The image is u8 (divided by 255 on the device, as the encoders' first layer does) or f32, image_bstride >= C*H*W
 * elements between consecutive images.
 *   var_convstack_n_params / _param_floats / _grad_offset   the published parameter order: weight (OIHW) and bias of every
 *       convolution in the module's state_dict order.  Gradient i lies at float offset var_convstack_grad_offset(kind, i) of
 *       the one flat grads_flat buffer, whose length is var_convstack_grad_offset(kind, n_params).
 *   var_convstack_saved_floats / _saved_offset   `saved` holds every convolution's post-ReLU map (B, C, H, H), un-pooled where
 *       a pool follows, in layer order: map j at float offset var_convstack_saved_offset(kind, B, j), j = n_params / 2 gives
 *       the length.  The last map equals feat.  Every offset is a multiple of four floats: there are no gaps.
 *   var_convstack_fwd   `params`: a HOST array of n_params device pointers in the published order (the reference's Policy has no
 *       arena).  One launch per convolution, one per pool, one copy.  saved may be NULL (a forward nobody differentiates: the
 *       maps then live in the workspace).
 *   var_convstack_bwd   given d_feat (B, 1152 | 288) and the `saved` of the forward over the same params and image: every
 *       weight and bias gradient into grads_flat, stored, not accumulated.  There is NO gradient for the image or the occupancy
 *       map -- the observations carry none in PPO -- so the first convolution has no data-gradient launch.  The pool backward
 *       routes a cell's gradient to the first maximum of its window in scan order and drops it where that maximum is not
 *       positive (PyTorch's rule).  Split-K partial sums go to the workspace and are added in slab order by fold launches; the
 *       split is a function of the shape alone.  No atomics: equal inputs give equal bits.
 * Stream-ordered, never synchronise, never allocate, read nothing back from the device (capturable).  Limits: B in 1..1024.
 * The gather-GEMM engine addresses an operand by 32-bit byte offsets from its base and divides k (and pixel) indices below
 * 2^24: at B = 1024 the largest operand, a (B, 32, 96, 96) map, is 1.2e9 bytes and the largest index, B * 96 * 96, is 9.4e6.
 * VAR_ERR_ARG, with a message that starts with the entry's name and nothing launched or written: kind not 0..2, B outside
 * 1..1024, a NULL pointer other than `saved` of the forward (a NULL entry of params included), image_bstride below C*H*W or a
 * batch of images of 4 GB or more, a workspace smaller than var_convstack_workspace_bytes, feat / saved / grads_flat /
 * workspace not 16-byte aligned.  The queries return VAR_ERR_ARG for a refused kind, index or B.
 *
 * The _ex entries add `flags` and, for the backward, `d_saved`; the entries without _ex are the _ex entries called with
 * flags = 0 and d_saved = NULL, and give the bits they always gave.
 *   flags bit 0: bf16 operands, for kinds 0 and 1.  Every convolution product, in all three directions, multiplies operands
 *       rounded to bf16 (round to nearest even) and accumulates in fp32; everything stored stays fp32 and every layout stays
 *       as it is (feat, saved, grads_flat, their offsets, the parameter order).
 *         forward, layer l   relu(conv(bf16(x_l), bf16(w_l)) + b_l): x_1 is the float image exactly as the fp32 path forms it
 *                            from bytes, x_l the (pooled) fp32 map below; the bias is added in fp32, pools act on the stored
 *                            fp32 maps.
 *         data gradient      conv_transpose(bf16(g_l), bf16(w_l)), g_l the fp32 gradient wrt layer l's pre-activation (what
 *                            the backward holds after the ReLU gate or the pool + ReLU backward).  Gates and pool routing are
 *                            exact selections on fp32 values by the rules above.
 *         weight gradient    the sum over pixels of bf16(g_l) * bf16(x_l); fp32 partial sums, slabs added in a fixed order
 *                            that depends on the shape alone; stored, not accumulated.
 *         bias gradient      fp32 channel sums of the unrounded g_l, as without the flag.
 *       Kind 2 accepts the flag and computes in fp32, bit for bit as without it.  Parameters, gradients, Adam state, the
 *       trunk, the head, the optimiser and the acting forwards are untouched by the mode.  Two sets of kernels serve it with
 *       these semantics (csrc/convstack.hip): the gather-GEMM with its operands rounded on the way into
 *       v_mfma_f32_32x32x16_bf16, and csrc/img_bf16.hip's kernels for the stride-1 padded layers behind conv 1 where they
 *       have an instantiation of the shape (their filter tables are packed inside every call into the workspace).
 *       Any other flag bit is refused.
 *   d_saved (may be NULL): `saved`'s layout and offsets.  When given, the backward writes every layer's g_l there instead of
 *       into its ping-pong workspace regions: g_l is the gated gradient with respect to the un-pooled map of convolution l,
 *       the operand that layer's weight and data gradients consume.  In both precisions, for every kind; grads_flat has the
 *       same bits with and without it.
 *   var_convstack_workspace_bytes_ex   the workspace the _ex entries need at those flags (VAR_ERR_ARG for a refused flag bit).
 * Refused like the rest (VAR_ERR_ARG, the entry's name first, nothing launched or written): a flag bit other than bit 0, a
 * d_saved that is not 16-byte aligned, a workspace shorter than var_convstack_workspace_bytes_ex reports for those flags. */
int var_convstack_n_params(int kind);
long var_convstack_param_floats(int kind, int i);
long var_convstack_grad_offset(int kind, int i);
long var_convstack_saved_floats(int kind, int B);
long var_convstack_saved_offset(int kind, int B, int j);
long var_convstack_workspace_bytes(int kind, int B);
int var_convstack_fwd(var_ctx* ctx, void* stream, int kind, const float* const* params, const void* image, int image_is_u8,
                      long image_bstride, int B, float* feat, float* saved /* may be NULL */, void* workspace,
                      long workspace_bytes);
int var_convstack_bwd(var_ctx* ctx, void* stream, int kind, const float* const* params, const void* image, int image_is_u8,
                      long image_bstride, int B, const float* saved, const float* d_feat, float* grads_flat, void* workspace,
                      long workspace_bytes);
long var_convstack_workspace_bytes_ex(int kind, int B, int flags);
int var_convstack_fwd_ex(var_ctx* ctx, void* stream, int kind, const float* const* params, const void* image, int image_is_u8,
                         long image_bstride, int B, float* feat, float* saved /* may be NULL */, void* workspace,
                         long workspace_bytes, int flags);
int var_convstack_bwd_ex(var_ctx* ctx, void* stream, int kind, const float* const* params, const void* image, int image_is_u8,
                         long image_bstride, int B, const float* saved, const float* d_feat, float* grads_flat, void* workspace,
                         long workspace_bytes, float* d_saved /* may be NULL */, int flags);

/* The frozen iTHOR encoder's reward step at RL batch sizes -----------------------------------------------------------
 * What the vectorised-env wrapper asks of the frozen pretext model on every environment step
 * (Envs/vec_env/vec_pretext_normalize.py:82-101 getEmbeddings / calcReward, processAI2Thor :125-146): the image embedding,
 * the goal sound's embedding (computed on the first step of an episode and cached FOR THE WHOLE BATCH afterwards,
 * models/pretext/pretext_base.py:26-32 "assuming every env reset at the same time") and their row dot.  The model is
 * models/pretext/ai2thor_pretext_model.py:5-58; params = the var_ithor_param_count() floats of var_ithor_encoder_fwd.
 * Inference only and always fp32, whatever var_ithor_set_bf16 says; nothing of the training path (its workspace, its bf16 /
 * GRU-sequence switches, its saved forward) is read or written, and a later var_plan / var_ithor_plan /
 * var_ithor_policy_plan at any batch leaves a captured reward graph valid: the plan owns every buffer it uses.
 *   var_ithor_reward_plan  (ai2thor_pretext_model.py:14-30: the 96x96 stack; Envs/ai2thor/RL_env_VAR.py:484 resizes to 96
 *       unconditionally): img_hw must be 96 and 1 <= max_batch <= 64 (the band convolutions' limit), else VAR_ERR_ARG --
 *       other sizes keep using var_ithor_encoder_fwd.  Only grows; a superseded block stays alive until var_destroy.
 *   var_ithor_reward_pack  (the encoder is frozen, VAR/RL_VAR.py loads it once): copies the arena into the plan's memory
 *       and lays conv 2..6 out for the matrix cores ONCE.  Every step reads that snapshot: parameters changed in place
 *       afterwards (load_state_dict) take effect at the next pack, not before, and packing again is all a checkpoint load
 *       needs -- the snapshot's address does not move, so captured graphs follow it.
 *   var_ithor_reward_step  (pretext_base.py:10-41 + calcReward): image (B,3,96,96) u8 (divided by 255) or f32,
 *       image_bstride >= 3*96*96 elements between images; goal_mfcc (B,1,600,40) or NULL.  With goal_mfcc: goal_feat (B,3)
 *       is written; with NULL it is read (the cached embedding).  image_feat (B,3) and reward (B) = sum_d image_feat *
 *       goal_feat are always written.  params must be the arena of the last pack (VAR_ERR_STATE otherwise, and before any
 *       pack); VAR_ERR_PLAN before the plan or beyond its batch.  A failed call launches nothing.
 * Launches (a captured step replays as this many kernel nodes): image only 7 (conv 1, four band convolutions with their
 * pool, the stride-2 conv 6, one tail: both Linear layers, F.normalize and the dot); with a goal 7 + 3 convolutions + the
 * input projection + 73 GRU steps (one launch each up to 16 clips: recurrent product of both directions, b_hh, gates and h'
 * fused; two launches each beyond, 72 products) + the 3 Linear layers of the sound head.  No kernel waits for another
 * workgroup: there is no time-out and no status word.
 *
 * config.RLRewardSoundSound (vec_pretext_normalize.py:82-101: the wrapper also embeds O['current_sound'] on EVERY step and
 * rewards <image_feat, goal_feat> + <current_sound_feat, goal_feat>):
 *   var_ithor_reward_plan_ex  var_ithor_reward_plan with flags; var_ithor_reward_plan is flags 0 and reserves what it always
 *       did.  VAR_IREW_SOUND_SOUND (bit 0) plans for max(max_batch, min(2 * max_batch, 16)) rows -- room for the goal and the
 *       current clips of up to 8 envs in ONE pass of the sound branch -- and reserves craw, the current clips' head output.
 *       Other bits: VAR_ERR_ARG.  A plan made with the bit serves every call; one made without it is replaced (never shrunk)
 *       when the bit is asked for, and the weights must be packed again.
 *   var_ithor_reward_step_ex  cur_mfcc = NULL: var_ithor_reward_step -- same launches, same bits, cur_feat / reward_img /
 *       reward_snd untouched.  With cur_mfcc (B,1,600,40), VAR_ERR_PLAN unless the plan has bit 0 and VAR_ERR_ARG without
 *       cur_feat: cur_feat (B,3) = the current clips' embedding, reward_img = sum_d image_feat * goal_feat, reward_snd =
 *       sum_d cur_feat * goal_feat (each where not NULL), reward = reward_img + reward_snd in one fp32 add: var_reward_dots'
 *       grouping.  The clips run through the goal clips' kernels, which treat clips independently, on the route
 *       var_ithor_reward_step takes for B clips -- a clip's embedding has the bits it has as a goal clip at the same B:
 *         goal and current clips, 2B <= 16: ONE pass of 2B clips (conv 1 once per clip set, then one launch per layer and one
 *             per GRU time step for both: 8 envs fill the fused step's 16 columns); goal rows 0..B-1, current rows B..2B-1
 *             of every sound buffer, the current clips' head output in graw rows B..2B-1;
 *         otherwise: one pass of B clips per clip set over the same buffers (the current clips last: the buffers hold theirs
 *             afterwards), the current clips' head output in craw.
 *       The tail stays one launch: its last workgroup also normalises the current clips' embedding and forms both dots.
 *       Launches: 7 + one sound pass (80 up to 16 clips) for a current-only step; 7 + 81 for a merged goal step; 7 + two
 *       passes otherwise. */
#define VAR_IREW_SOUND_SOUND 1
int var_ithor_reward_plan(var_ctx* ctx, int max_batch, int img_hw);
int var_ithor_reward_plan_ex(var_ctx* ctx, int max_batch, int img_hw, int flags);
int var_ithor_reward_step_ex(var_ctx* ctx, void* stream, const float* params,
                             const void* image, int image_is_u8, long image_bstride,
                             const float* goal_mfcc /* | NULL */, const float* cur_mfcc /* | NULL */, int B,
                             float* image_feat, float* goal_feat, float* cur_feat, float* reward,
                             float* reward_img /* | NULL */, float* reward_snd /* | NULL */);
int var_ithor_reward_pack(var_ctx* ctx, void* stream, const float* params);
int var_ithor_reward_step(var_ctx* ctx, void* stream, const float* params,
                          const void* image, int image_is_u8, long image_bstride,
                          const float* goal_mfcc, int B,
                          float* image_feat, float* goal_feat, float* reward);
/* The sound embeddings from a device clip table.  The env's sounds come from a finite, unaugmented pool (Envs/audioLoader.py:
 * 166-237: a stored clip picked by index, the all-zero matrix when nothing is heard) and the encoder is frozen, so a clip's
 * embedding is a constant of (checkpoint, clip): embed the pool once, then a step gathers rows by id instead of running the
 * sound branch.
 *   var_ithor_reward_embed  mfcc (n,1,600,40) f32 -> out (n,3), any n >= 1, with the packed snapshot: the sound branch over the
 *       plan's own buffers in passes of at most min(16, plan rows) clips -- always the fused one-launch GRU step -- and after
 *       each pass one small kernel that normalises the pass's head outputs with the tail's expression.  Needs a plan and a pack,
 *       params == the packed arena (VAR_ERR_PLAN / VAR_ERR_STATE as var_ithor_reward_step; mfcc / out NULL or n < 1:
 *       VAR_ERR_ARG); a refused call launches nothing.  No allocation; capturable.  Row i has the bits var_ithor_reward_step_ex
 *       writes to cur_feat and var_ithor_reward_step to goal_feat for the same clip at any B up to 16 clips a pass, whichever
 *       clips share its pass: no kernel of the branch mixes clips.  Launches: 81 per pass.
 *   var_ithor_reward_step_ids  the image stack's six launches + ONE tail, 7 kernels on every kind of step; the tail's finishing
 *       thread of a row gathers from table (table_rows, 3) instead of normalising head outputs.  goal_ids (B) i32 on the
 *       device | NULL: id g >= 0 takes table[g] and writes it to goal_feat[row]; g == -1 reads goal_feat[row], the embedding
 *       cached for THAT env (an env that starts an episode alone gets its new goal without the others re-sending theirs); NULL
 *       = every row -1.  cur_ids (B) i32 on the device | NULL: cur_feat[row] = table[c], reward = <image, goal> + <current,
 *       goal> in var_reward_dots' grouping, reward_img / reward_snd where given; NULL: var_ithor_reward_step's image-only
 *       bits, cur_feat / reward_img / reward_snd untouched.  An id outside its range (goal < -1 or >= table_rows; current < 0
 *       or >= table_rows) is never turned into an address: that row's image_feat, cur_feat and rewards are NaN, its goal_feat
 *       stays as it was, other rows are unaffected.  The ids are read on the device: one captured graph serves goal steps,
 *       image-only steps and staggered resets.  Any plan serves (no VAR_IREW_SOUND_SOUND needed: no sound pass is reserved).
 *       VAR_ERR_PLAN / VAR_ERR_STATE / VAR_ERR_ARG as var_ithor_reward_step; also VAR_ERR_ARG: cur_ids without cur_feat, table
 *       NULL, table_rows < 1.  A failed call launches nothing. */
int var_ithor_reward_embed(var_ctx* ctx, void* stream, const float* params, const float* mfcc /* (n,1,600,40) */, int n,
                           float* out /* (n,3) */);
int var_ithor_reward_step_ids(var_ctx* ctx, void* stream, const float* params,
                              const void* image, int image_is_u8, long image_bstride,
                              const float* table, int table_rows,
                              const int* goal_ids /* (B) device | NULL */, const int* cur_ids /* (B) device | NULL */, int B,
                              float* image_feat, float* goal_feat, float* cur_feat, float* reward,
                              float* reward_img /* | NULL */, float* reward_snd /* | NULL */);

/* The iTHOR/FSC audio front-end: python_speech_features.mfcc as called at Envs/audioLoader.py:158-161 (pre-emphasis
 * .97, 400/160 frames with a zero-padded tail, np.hamming, |rfft_512|^2/512, 40 triangles, log, orthonormal DCT-II,
 * lifter 22, coefficient 0 = log frame energy; int16 samples NOT normalised) + processSoundFeat (:241-252).
 * Arguments as var_mfcc; T = 1 + ceil((len-400)/160) frames per clip (1 if len <= 400), out (nclips,1,out_frames,40)
 * f32 (the library computes float64; this kernel float32).  pcm_stride must be even (rows are read as 4-byte sample
 * pairs; an odd stride is refused with VAR_ERR_ARG, ops.mfcc_psf refuses an odd width).  The tables are built on the first call (the only
 * call of this entry that allocates: make it once outside graph capture). */
int var_mfcc_psf(var_ctx* ctx, void* stream, const int16_t* pcm, const int* lens, const int* clip_index,
                 int nclips, int pcm_stride, int out_frames, float* out);

/* Measurement and testing hooks -------------------------------------------------
 * var_profile_select: record HIP events, on the launch stream, around every launch of one
 * kernel family (tag in [0, var_profile_tag_count()), -1 = off); var_profile_read returns the
 * summed durations and the launch count since the select (it synchronises on the events).
 * var_set_streams: which parts of a step leave the caller's stream (bit 0: sound branch forward incl. the in-step MFCC, bit 1:
 * sound CNN backward, bit 6: the training step's forward and backward hand over between their two streams with graph edges
 * again instead of device-side flags, see var_join_status; bit 7: under a clip cache the step's front-end copies served clips
 * into the feature buffer and zeroes empty ones, as before clips were read in place -- an opt-out that gives a bit-for-bit
 * reference inside one build, see var_mfcc_cache_bind; other bits are ignored); -1 restores the default (3).
 * 0 puts every kernel on the caller's stream (per-kernel timing).  Returns the previous mask, as stored: passing it back
 * restores it.
 * var_join_status: in a training step recorded under stream capture (var_arm_loss_grad* with all three branches, two
 * streams; launched eagerly the step keeps its stream edges) the backward's first kernels
 * do not wait for the other stream's forward through the streams (a barrier packet in a replayed graph costs ~10 us there):
 * the last workgroup of each branch's last forward kernel counts a flag up and polls the other branch's before it ends; a
 * poll gives up after 5 ms -- the other branch never ran: a fault, the step's numbers are undefined -- and counts itself.
 * *timeouts = that count since var_init (synchronous copy; the reference's loss.backward(), VAR/pretext_VAR.py:68, has no
 * such failure mode, so it is reported).
 * var_debug_buffer: address/length of a named workspace buffer ("act1".."act5", "gact1"..,
 * "sact1".."sact4", "gsact1".., "emb", "gemb", "wpack"; "ithor_s1".."ithor_s3", "ithor_gs1".."ithor_gs3") for
 * layer-wise parity tests.  The Kuka heads' rows: "hid_i" (B, 128) and "hid_s" (positive clips from row 0, negative ones
 * from row B, 128 floats each); the others are (3 maxB) stacks [image | positive | negative] that a call of B samples fills
 * with B-BASED offsets (image rows from row 0, positive clips from row B, negative ones from row 2B): "emb" / "emb_raw" (rows
 * of 3: the normalised and the un-normalised embeddings), "head_part" (rows of 16: the four partial sums of the 128 -> 3
 * layer, 4 floats each, the fourth unused; img_mid3 leaves an image's whole sum in the first group), "gemb" (rows of 3),
 * "graw" (rows of 4: the gradient wrt emb_raw and a zero) and "ghid" (rows of 128: the masked hidden gradient); graw and
 * ghid are written by var_arm_encoder_bwd and by the training step above 1024 rows per head -- below that the fused step
 * forms them in registers only.
 * The iTHOR model's names, after the "ithor_" prefix (lengths are those of the PLAN's batch; the
 * saved forward fills the first B images | nclips clips of each, sound-side strides by nclips): a1..a6, p2..p5, ga1..ga6,
 * gp2..gp5 (image maps, pooled maps, gradients), s1..s3, gs1..gs3 (sound maps; 3 in the (clip, 73, 64, 7) sequence layout),
 * gi (dir, clip*73 + t, 1536), hb (dir, step 0..73, clip, 512), gh (split-K partials), dgi (as gi), dgh (dir, step, clip,
 * 1536), sraw / gsraw (clip, 1024), hid_i / ghid_i (B, 128), hid_s1 / ghid_s1 (clip, 128), hid_s2 / ghid_s2 (clip, 64),
 * raw / graw / emb (3*maxB rows of 3: images from row 0, clips from row maxB).
 * The acting forwards' workspaces, after "arm_" (var_armnet_forward) / "ipol_" (var_ithor_policy_forward); lengths are
 * those of the PLAN's batch, a forward of B rows fills the first B rows of each with B-based strides: a1..a8 / a1..a6 (conv
 * outputs after ReLU, (B, C, h, h); up to 64 images the band kernels pool inside the launch and a2, a4, a6 / a2..a5 are not
 * written), p1..p3 / p1..p4 (pooled maps), ipol_ only: occf (B, 288), occ (B, 256), h1 (B, 1024); the per-layer path's (B > 8)
 * flat_img, motor, sound, fusion (B, 256), h0 = rnn_hxs * masks (B, H), gi, gh (B, 3H), t0..t3 (B, <= 512 scratch rows: what
 * its last writer left).  The small-batch chain's handed-over vectors under their schedule's names (CNN0, FLAT, M0, M1,
 * MOTOR, S0, S1, SOUND, O0, OCC, GH, IM0, X, F0, FUSION, GI, IMR, ALL0, ALL1, C0, C1, A0, AFT; known once a chain launch has
 * run on the plan): the raw area of 8 rows x width (value, tag) pairs, value in the low word, the launch's epoch in the
 * high word; "chain": the whole pair area; "sync": the chain's 64 sync words ([3] = the epoch of the next launch).
 * The reward plan's buffers (var_ithor_reward_plan / _pack / _step), after "irew_"; lengths are those of the PLAN's batch
 * maxB, VAR_ERR_PLAN before a plan, VAR_ERR_ARG for an unknown name.  A step of B rows fills the first B rows of a1 (B, 32,
 * 96, 96), p1..p4 (the fused conv + pool outputs: (B, 32, 48, 48), (B, 64, 24, 24), (B, 64, 12, 12), (B, 128, 6, 6)), a6
 * (B, 1152), hid (B, 128); a goal step also s1 (clip, 64, 300, 20), s2 (clip, 64, 150, 13), s3 in the sequence layout
 * (clip, 73, 448), gi (dir, clip*73 + t, 1536) with the direction stride B*73*1536, gh (the four split-K slabs of
 * h W_hh^T above 16 clips: (slab, dir, clip, 1536) with B-based strides), hb (the two state slots, maxB*1024 floats
 * apart, each (clip, [forward 512 | reverse 512]): slot 1 holds the last state h_73, slot 0 the one before), hs1 (clip,
 * 128), hs2 (clip, 64), graw (clip, 3: the sound head before F.normalize), craw (clip, 3: the same of the current clips of a
 * sound-sound step that ran them in a pass of their own; a merged pass leaves them in graw rows B..2B-1; zero floats long
 * without VAR_IREW_SOUND_SOUND); frozen: the parameter snapshot of the last var_ithor_reward_pack (var_ithor_param_count()
 * floats).
 * var_debug_ithor_dense: one dense product of the iTHOR model's bf16 mode through the kernel its schedule would pick,
 * C[m + n*M] (+= when `add`) = sum_k A(m,k) B(k,n), A(m,k) = a[m*K + k] if a_kfast else a[k*M + m], B likewise with
 * b[n*K + k] | b[k*N + n]; nsplit > 1 writes split-K slabs C + s*M*N instead (device pointers, fp32).  Returns 1 when
 * the staged bf16 kernel (dense_bf16.h) ran, 0 when the shapes fell back to the gather-GEMM, < 0 on error.  `add` bit 1:
 * both operands are first copied to bf16 and handed over as copies, as the model's schedule does for its big products
 * (nsplit must be 1); then 2 is returned when the resident-panel kernel (K = 448, both operands k-fast) took it. */
int var_profile_tag_count(void);
const char* var_profile_tag_name(int tag);
int var_profile_select(var_ctx* ctx, int tag);
int var_profile_read(var_ctx* ctx, float* total_ms, int* count);
int var_set_streams(var_ctx* ctx, int mask);
int var_join_status(var_ctx* ctx, unsigned* timeouts);
int var_debug_buffer(var_ctx* ctx, const char* name, void** ptr, long* nfloats);
/* tests: the next persistent GRU forward is launched one workgroup short per hand-off group, so that no group can
 * complete -- what the resident part of a grid sees when the rest is not: every wait must expire (about 0.3 s), the
 * launch must end, var_ithor_gru_status must read non-zero and the step's outputs must be NaN. */
int var_debug_ithor_gru_drop_workgroup(var_ctx* ctx);
/* tests: the next small-batch chain launch of var_armnet_forward runs one workgroup short: the vectors that workgroup owes never
 * arrive, every consumer's wait must expire (about 0.3 s), the launch must end with NaN outputs, var_armnet_status must read 1,
 * and the launch after that must be clean (status 0x40000001 until cleared). */
int var_debug_armnet_drop_workgroup(var_ctx* ctx);
int var_debug_ithor_dense(var_ctx* ctx, void* stream, int a_kfast, int b_kfast, const float* a, const float* b,
                          float* c, int M, int N, int K, int nsplit, int add);
/* timing (tools/mfcc_time.py): the front-end launch that var_arm_loss_grad_pcm makes under a clip cache, on its own --
 * 100 output frames, served and empty slots of `out` (16-byte aligned) are left as they are, live ones written.
 * VAR_ERR_STATE without a binding for this pcm / pcm_stride. */
int var_debug_mfcc_in_place(var_ctx* ctx, void* stream, const int16_t* pcm, const int* lens, const int* clip_index,
                            int nclips, int pcm_stride, float* out);

#ifdef __cplusplus
}
#endif
#endif /* VAR_HIP_H */
