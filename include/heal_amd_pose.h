/* heal_amd_pose.h -- CoAlign's agent-object pose graph (box alignment): every agent's stage-1 boxes, with their uncertainties,
 * correct the agents' noisy relative poses before fusion.  Reference: box_alignment_relative_sample_np,
 * opencood/models/sub_modules/box_align_v2.py:105-400, with the g2o optimiser of pose_graph_optim.py replaced by a
 * Levenberg-Marquardt solve on the same cost inside the kernel.  The host mirror (numpy float64, the same steps) is
 * heal_amd/opencood/models/sub_modules/{box_align_v2,pose_graph_optim}.py; DESIGN.md section 28 holds the contract.
 *
 * The inference ABI (include/heal_amd.h, HEAL_AMD_ABI_VERSION) stays as it is; the entry points declared here are shipped in the
 * same library (every build exports them).  Same conventions as include/heal_amd.h: device pointers read where they lie, a
 * hipStream_t as void*, non-zero return + heal_last_error() on failure, kernel launches only and no host synchronisation (safe
 * under graph capture), no floating-point atomics, a workspace that need not be initialised, *_workspace / *_supported are host
 * arithmetic and return 0 for a shape out of range.  All geometry and the solve are fp64.
 *
 * One launch handles a batch of S samples; a sample's result depends on nothing outside the sample (bit-equal alone or inside any
 * batch, and across repeated launches).  Two kernels: a pass over all boxes (both corner_to_center's and the 6-DoF projection into
 * the world frame), then one 256-thread workgroup per sample that clusters the boxes into landmarks (sequential over seeds, each
 * seed's neighbour test across the lanes against a bit set of unassigned boxes in LDS) and runs the whole solve: per iteration one
 * thread per landmark accumulates its 3x3 block, right-hand side and coupling blocks, the Schur complement onto the 3 (N - 1)
 * agent unknowns is summed over landmarks in index order, a dense Cholesky with the LM damping is factored in LDS, and each
 * landmark back-substitutes its own update.  Every loop is bounded independently of the data: seeds <= boxes, iterations <=
 * max_iterations <= HEAL_POSE_MAX_ITERATIONS, trial steps <= 10 per iteration.
 *
 * Graph, cost, damping and stopping rule: heal_amd/opencood/models/sub_modules/pose_graph_optim.py (module docstring).  The
 * quirks of the reference's graph construction are kept (non-transitive greedy clustering in box order, sqrt(a^2 + b^2 - 2ab)
 * distances whose NaN compares false, the plain mean of four arctan2 as a box's yaw, certainties doubled for a yaw-varying
 * cluster under adaptive_landmark) except one: the reference's world frame is float32 (its pose_to_tfm / project_box3d round a
 * numpy input), this one is fp64.
 */
#ifndef HEAL_AMD_POSE_H
#define HEAL_AMD_POSE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HEAL_POSE_MAX_AGENTS 8          /* agents per sample                                                     */
#define HEAL_POSE_MAX_BOXES 1024        /* boxes per sample (all agents): the per-box tables of a sample fit LDS */
#define HEAL_POSE_MAX_ITERATIONS 1000   /* max_iterations is clamped to this (the reference's default)           */
#define HEAL_POSE_STATS 8               /* doubles per sample in `stats`                                         */

/* option bits */
#define HEAL_POSE_LANDMARK_SE2 1
#define HEAL_POSE_ADAPTIVE_LANDMARK 2
#define HEAL_POSE_NORMALIZE_UNCERTAINTY 4
#define HEAL_POSE_ABANDON_HARD_CASES 8
#define HEAL_POSE_DROP_HARD_BOXES 16
#define HEAL_POSE_DROP_UNSURE_EDGE 32

/* stats[s * HEAL_POSE_STATS + ...] */
#define HEAL_POSE_STAT_LANDMARKS 0      /* clusters created                                                      */
#define HEAL_POSE_STAT_EDGES 1          /* edges in the graph (active landmarks, not dropped as unsure)          */
#define HEAL_POSE_STAT_ITERATIONS 2     /* outer LM iterations run                                               */
#define HEAL_POSE_STAT_STATUS 3         /* one of HEAL_POSE_STATUS_*                                             */
#define HEAL_POSE_STAT_CHI2_INITIAL 4
#define HEAL_POSE_STAT_CHI2_FINAL 5
#define HEAL_POSE_STAT_LAMBDA 6         /* the damping when the solve ended                                      */
#define HEAL_POSE_STAT_TRIALS 7         /* trial steps solved in total                                           */

#define HEAL_POSE_STATUS_CONVERGED 0        /* ended by the stopping rule                                        */
#define HEAL_POSE_STATUS_MAX_ITERATIONS 1
#define HEAL_POSE_STATUS_NO_EDGES 2         /* nothing to optimise: the noisy poses are the result               */
#define HEAL_POSE_STATUS_ABANDONED 3        /* abandon_hard_cases: the noisy poses are the result, bit for bit   */
#define HEAL_POSE_STATUS_NONFINITE 4        /* a non-finite corner, pose, uncertainty or cost: the noisy poses   */

/* heal_pose_graph_supported (host only): 1 if a sample of this size is taken -- 1 <= agents <= HEAL_POSE_MAX_AGENTS and
 *   0 <= boxes <= HEAL_POSE_MAX_BOXES -- else 0.                                                                */
int heal_pose_graph_supported(int max_agents_per_sample, int max_boxes_per_sample);

/* bytes of workspace of heal_pose_graph_align; 0 for a shape out of range */
size_t heal_pose_graph_workspace(int samples, int total_agents, int total_boxes);

/* heal_pose_graph_align, all pointers device memory except where said:
 *   corners        f64 [M, 8, 3]            every agent's boxes in its own frame, concatenated in agent order
 *   box_offsets    i32 [total_agents + 1]   agent a's boxes are rows box_offsets[a] .. box_offsets[a + 1]
 *   agent_offsets  i32 [samples + 1]        sample s's agents are agent_offsets[s] .. agent_offsets[s + 1]; the first is its ego
 *   lidar_pose     f64 [total_agents, 6]    x, y, z, roll, yaw, pitch in degrees (CARLA convention)
 *   log_sigma2     f64 [M, 3] or NULL       log variance of (x, y, yaw) per box; NULL = use_uncertainty False
 *   max_agents, max_boxes                   host: the largest sample of the batch (what the caller checked with _supported);
 *                                           a sample that exceeds either on the device ends with status NONFINITE
 *   options        HEAL_POSE_* bits;  thres, yaw_var_thres, max_iterations as in the reference
 *   refined        f64 [total_agents, 3]    x, y, yaw in degrees, the yaw in (-180, 180].  A vertex the solve did not move (the
 *                                           ego, an agent without an active edge) keeps its x, y and -- with its yaw already in
 *                                           (-180, 180] -- its yaw bit for bit.
 *   cluster_of_box i32 [M] or NULL          -1, or the landmark's index within its sample in creation order
 *   stats          f64 [samples, HEAL_POSE_STATS] or NULL
 *   ws             heal_pose_graph_workspace bytes, 256-B aligned, need not be initialised                        */
int heal_pose_graph_align(const double* corners, const int32_t* box_offsets, const int32_t* agent_offsets,
                          const double* lidar_pose, const double* log_sigma2, int samples, int total_agents, int total_boxes,
                          int max_agents, int max_boxes, int options, double thres, double yaw_var_thres, int max_iterations,
                          double* refined, int32_t* cluster_of_box, double* stats, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
