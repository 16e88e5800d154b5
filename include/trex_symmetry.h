/*
 * trex_symmetry.h - C-ABI of the mirror maps of the device trainer: a signed permutation of the columns of a row block, applied on
 * the device to observation rows, critic rows and action blocks alike; the mirrored half of a rollout appended behind the real
 * one; the running observation moments made those of the augmented stream. K22.
 *
 * The table and the two row launches know neither a batch nor a policy: they read and write plain device buffers. Only
 * trex_policy_symmetrize_stats takes a TrexPolicy (include/trex_policy.h).
 *
 * Conventions as in trex_batch.h and trex_policy.h: 0 / negative TREX_E_* codes (TREX_OK 0, TREX_E_INVALID -1, TREX_E_HIP -5),
 * trex_last_error(), caller-owned device buffers that are validated once per allocation, stream-ordered asynchronous launches
 * (void* = hipStream_t), capturable from the second call with the same buffers on. On TREX_E_INVALID nothing is launched and
 * nothing is changed.
 *
 * Semantics (ONE definition).
 *
 * Model (trex_model_mirror_table, host only). The sagittal plane passes through the origin of URDF link 0 and its normal is the axis
 *   `lateral` (0, 1 or 2) of link 0's frame; S negates that component. Every body's frame at q = 0 is taken in link 0's frame; a
 *   body's origin is its joint's (body 0, the base: link 0's). Body i is its own pair where |S o_i - o_i| <= tol_pos, else its pair
 *   is the body j != i with the smallest |S o_i - o_j| <= tol_pos (the lowest j among equals). The sign of a joint is the sign of
 *   a_i . (-S a_j), j its pair: an axis reflects as an axial vector (0 counts as +). Joints are in observation order (sorted names),
 *   as everywhere else. Refused, TREX_E_INVALID: a body without a partner, a pairing that is no involution, paired bodies whose
 *   parents are not paired, limits [lower_i, upper_i] that differ from the image of the pair's - [lower_j, upper_j] for sign +,
 *   [-upper_j, -lower_j] for sign - - by more than tol_pos rad. lateral -1 searches: the first of the axes 0, 1, 2 that is not
 *   refused and pairs some body with another one; where none does, the first that is not refused.
 *   residual_out says what is NOT symmetric and refuses nothing: [0] the largest |m_i - m_j| / max(m_i, m_j) of a pair, [1] the
 *   largest |o_i - S o_j| in metres, [2] the largest angle in radians between a_i and +-(-S a_j), [3] the largest |c_i - S c_j| of
 *   the bodies' centres of mass at q = 0, [4] the distance of the base's centre of mass from the plane.
 *
 * Row table (trex_model_mirror_row_table, host only). The table of the composed row of include/trex_batch.h,
 *   [q J | qd J | torque J | the E channel columns | tail], tail = 2 (reward, done) or 5 (with the penalties). Base axes are URDF
 *   link 0's frame, the frame `lateral` is an axis of.
 *     q, qd, torque blocks                                              the joint table
 *     PROJECTED_GRAVITY, BASE_LINEAR_VELOCITY, POINT_POSITION, POINT_VELOCITY   polar vectors: the lateral component changes sign
 *     BASE_ANGULAR_VELOCITY                                             an axial vector: the two other components change sign
 *     BASE_HEIGHT, POINT_HEIGHT, CONTACT_FORCE                          unchanged
 *     PREV_ACTION                                                       the action table, within the channel
 *     EXTERNAL                                                          the caller's extern_src / extern_sign: a table over the
 *                                                                       EXTERNAL columns of the row, concatenated in channel order
 *     tail                                                              maps to itself
 *   A POINT_* or CONTACT_FORCE channel maps to the first channel of the same kind and scale whose link lies in the body paired with
 *   its own link's body; for the POINT_* kinds the partner's point at q = 0 must be the image of its own within tol_pos. Where the
 *   specification has no such channel: TREX_E_INVALID, the message names the channel index. An EXTERNAL channel without extern_src
 *   and extern_sign, or with an extern_src that is no permutation: TREX_E_INVALID.
 *
 * Action table. [A]: the joint table; with stiffness actions (A = 2 J) a second block of the same permutation, offset by J, sign +1.
 * Command table. A velocity command (vx, vy, wz) in base axes maps to itself with the lateral component and wz negated (wz is the
 *   z component of an axial vector: it keeps its sign only for lateral 2).
 *
 * Table. A mirror table of width W, 1 <= W <= TREX_MIRROR_MAXWIDTH (517, the widest composed row), is src[W] and sign[W]: src is a
 *   permutation of [0, W), sign[c] is +1 or -1. The mirror image of a row x [W] is the row y [W] with
 *       y[c] = sign[c] * x[src[c]].
 *   "sign[c] * v" is no float arithmetic: where sign[c] < 0 the sign BIT of v is flipped, else v is copied. So the image is defined
 *   bit for bit for every input - a NaN keeps its payload, +0 and -0 change places, an infinity changes its sign. A table need not
 *   be an involution; the tables of a mirror symmetry are (src[src[c]] == c and sign[src[c]] == sign[c]), and applying such a table
 *   twice reproduces the input bit for bit.
 *
 * Rows (trex_mirror_rows). out[e stride_out + c] = sign[c] * in[e stride_in + src[c]] for e < n, c < W. Nothing else of an out row
 *   is written: the columns W .. stride_out - 1 keep what they held. in == out with equal strides is allowed: every row is read
 *   completely before any of it is stored. Any other overlap of the two blocks is refused.
 *
 * Augment (trex_mirror_augment). The rollout buffers of include/trex_policy.h are flat arrays over samples: obs [., D], act [., A],
 *   logp, val, adv, ret [.], and with a privileged critic obs_v [., Dv], rows packed (stride = width). With N = num_samples, ONE
 *   launch fills the samples N .. 2N - 1 of every buffer from the samples 0 .. N - 1:
 *       obs[N + i] = image of obs[i] under the obs table, act[N + i] = image of act[i] under the act table,
 *       obs_v[N + i] = image of obs_v[i] under the critic table (where given),
 *       logp[N + i] = logp[i], val[N + i] = val[i], adv[N + i] = adv[i], ret[N + i] = ret[i]            (copies).
 *   The mirrored samples keep the log-probability, value, advantage and return of the originals. THIS TREATS THE ROLLOUT POLICY AS
 *   IF IT WERE SYMMETRIC - pi(M_a a | M_o s) = pi(a | s), V(M_o s) = V(s) -, which holds for no policy exactly: the importance
 *   ratio of a mirrored sample starts at pi_theta(M_a a | M_o s) / pi_old(a | s), not at 1. It is the augmentation of rsl_rl. The
 *   samples 0 .. N - 1 are not written.
 *
 * Moments (trex_policy_symmetrize_stats). VecNormalize's running moments of the observation block, mean[D] and var[D] in f64
 *   (trex_policy_get_stats: [mean D | var D | count | ..]), become those of the stream in which every row is followed by its image.
 *   For a column c with c' = src[c], s = sign[c], every value read before any is written, every operation rounded to f64, in this
 *   order and without contraction into fused multiply-adds:
 *       a = s * mean_old[c']                      (the sign bit)
 *       mean[c] = (mean_old[c] + a) / 2
 *       h = (mean_old[c] - a) / 2
 *       var[c] = (var_old[c] + var_old[c']) / 2 + h * h
 *   The count and the return moments are not touched. For an involution table the call is idempotent bit for bit: after it
 *   mean[c] == s mean[c'] and var[c] == var[c'], so a second call changes nothing. The f32 image of the moments that
 *   trex_policy_act normalises with is refreshed as trex_policy_set_stats refreshes it; after the call, normalising a row commutes
 *   with mirroring it, bit for bit, which is what lets the augment launch work on the stored NORMALISED observations. With a critic
 *   table the moments of the critic's rows (trex_policy_critic_get_stats) are treated alike.
 */
#ifndef TREX_SYMMETRY_H
#define TREX_SYMMETRY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define TREX_MIRROR_MAXWIDTH 517

typedef struct TrexMirrorTable TrexMirrorTable;
struct TrexPolicy;
struct TrexModel;

/* Host only: no device is touched. pair_out [J], sign_out [J], body_pair_out [B], residual_out [5], lateral_out: each nullable;
 * lateral_out receives the axis in force. TREX_E_INVALID: a NULL model, lateral outside -1 .. 2, a tol_pos that is negative or not
 * finite, and the refusals of the semantics - the message names the body or joint. */
int trex_model_mirror_table(const struct TrexModel *model, int lateral, double tol_pos, int32_t *pair_out, int8_t *sign_out,
                            int32_t *body_pair_out, double *residual_out, int *lateral_out);
/* Host only. channels_host: TrexObsChannel [num_channels] of include/trex_batch.h (passed as void*: this header includes no other);
 * action_cols: J or 2 J; tail: 2 or 5; extern_src, extern_sign nullable without an EXTERNAL channel; src_out, sign_out [3 J + E +
 * tail], width_out (nullable) <- that width. The model table is that of (lateral, tol_pos), lateral -1 searched. TREX_E_INVALID:
 * what trex_model_mirror_table refuses, an unknown kind, a link out of range, a row wider than TREX_MIRROR_MAXWIDTH, and the
 * refusals of the semantics. */
int trex_model_mirror_row_table(const struct TrexModel *model, int lateral, double tol_pos, const void *channels_host, int num_channels,
                                int action_cols, int tail, const int32_t *extern_src, const int8_t *extern_sign, int32_t *src_out,
                                int8_t *sign_out, int *width_out);
/* Host only. pair, sign: a joint table [J]; src_out, sign_out: [J], or [2 J] with stiffness != 0. */
int trex_mirror_action_table(const int32_t *pair, const int8_t *sign, int num_joints, int stiffness, int32_t *src_out, int8_t *sign_out);
/* Host only. src_out, sign_out: [3]. TREX_E_INVALID: lateral outside 0 .. 2. */
int trex_mirror_command_table(int lateral, int32_t *src_out, int8_t *sign_out);

/* A device copy of src_host [width] and sign_host [width] (host arrays, copied; a set-up call: it synchronises). TREX_E_INVALID: a
 * NULL argument, a width outside [1, TREX_MIRROR_MAXWIDTH], a src that is no permutation of [0, width) - the message names the
 * column -, a sign that is neither +1 nor -1, a device that does not exist. */
int trex_mirror_table_create(const int32_t *src_host, const int8_t *sign_host, int width, int device, TrexMirrorTable **out);
void trex_mirror_table_destroy(TrexMirrorTable *table);
/* The width (nullable) and whether the table is an involution (nullable: 1 or 0). */
int trex_mirror_table_info(const TrexMirrorTable *table, int *width, int *involution);

/* ONE launch. Strides in floats. TREX_E_INVALID: a NULL argument, n < 1, width != the table's, a stride below the width, n * stride
 * beyond 2^31, blocks that overlap other than in_dev == out_dev with in_stride == out_stride, host memory or another device's, a
 * short buffer. */
int trex_mirror_rows(TrexMirrorTable *table, const float *in_dev, int in_stride, float *out_dev, int out_stride, int n, int width,
                     void *stream);

/* ONE launch. critic_table, obs_v_dev and Dv go together: all given, or NULL, NULL and 0. Every buffer holds 2 num_samples rows.
 * TREX_E_INVALID: a NULL argument among the required ones, num_samples < 1, D, A or Dv != its table's width, 2 num_samples * the
 * widest width beyond 2^31, tables of different devices, host memory or another device's, a buffer shorter than 2 num_samples
 * rows. The buffers are checked one by one, as everywhere in this C-ABI: buffers that alias EACH OTHER are not refused, and the
 * result of such a call is undefined. */
int trex_mirror_augment(TrexMirrorTable *obs_table, TrexMirrorTable *act_table, TrexMirrorTable *critic_table, float *obs_dev,
                        float *act_dev, float *logp_dev, float *val_dev, float *adv_dev, float *ret_dev, float *obs_v_dev,
                        int64_t num_samples, int D, int A, int Dv, void *stream);

/* Two launches (the moments, their f32 image), and two more with a critic table. critic_table nullable. TREX_E_INVALID: a NULL
 * policy or obs table, a table whose width is not the policy's obs_dim (critic table: not the critic width in force, or no critic is
 * set), a table on another device than the policy's. */
int trex_policy_symmetrize_stats(struct TrexPolicy *policy, const TrexMirrorTable *obs_table, const TrexMirrorTable *critic_table,
                                 void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* TREX_SYMMETRY_H */
