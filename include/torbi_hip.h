/*
 * torbi_hip.h -- C ABI of libtorbi_hip.so, the MI355X (gfx950) batched Viterbi decoder.
 *
 * This is the drop-in boundary for ONE path of maxrmorrison/torbi: the operator
 *
 *     torbi::viterbi_decode(Tensor observation, Tensor batch_frames,
 *                           Tensor transition, Tensor initial) -> Tensor
 *
 * declared at reference torbi/csrc/ops.cpp:16-18, implemented for CUDA at
 * torbi/csrc/cuda/viterbi.cu:309-362 (viterbi_decode_cuda) and called from
 * torbi/viterbi.py:53.  The entry points below are what a binding for that operator
 * binds; INTEGRATION.md shows the ctypes stub and the torch.library registration.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / ATen types
 *   - all pointers are DEVICE pointers on HIP device `device` unless stated otherwise
 *   - tensors are contiguous row-major (the reference calls .contiguous() itself,
 *     viterbi.cu:325-328)
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     device's default stream), performs no allocation, keeps no pointer after return, and
 *     is re-entrant across devices/streams
 *   - return value: 0 = success, < 0 = argument error (TORBI_HIP_E*), > 0 = a hipError_t
 *     reported by the runtime (launch failure etc.)
 *
 * Result contract (what "same results as the reference" means; reference CPU path,
 * torbi/csrc/viterbi.cpp, line numbers in DESIGN.md):
 *   - transition is indexed [next, prev]; candidate(j,i) = fl(post[i] + transition[j*S+i])
 *   - post'[j] = fl(observation[t,j] + max_i candidate(j,i)); t = 0: fl(obs[0,i]+initial[i])
 *   - backpointer = LOWEST index attaining the maximum; final state = lowest index attaining
 *     the maximum of the last posterior row; every output position t >= batch_frames[b]-1
 *     holds that final state
 *   - decoded indices are bit-identical to the reference CPU operator, -inf, +inf and NaN
 *     inputs included: the reference is deterministic there (a NaN candidate at prev-state 0
 *     is never replaced and a NaN candidate elsewhere never wins, viterbi.cpp:94-100; the
 *     final state is ATen's argmax, the first NaN of the last row, :218), the fast kernels
 *     are not, so every decode looks for NaN / +inf in what it reads and produces and an
 *     item that met one is decoded again on the device in the reference's own order of
 *     evaluation (csrc/nonfinite.hpp: no host involvement, nothing to pay on finite inputs
 *     beyond two small launches).  batch_frames[b] outside [1, T] is clamped on the device
 *     (the reference reads out of bounds for 0, viterbi.cpp:153).
 */
#ifndef TORBI_HIP_H
#define TORBI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TORBI_HIP_ABI_VERSION 17

#define TORBI_HIP_OK 0
#define TORBI_HIP_EINVAL (-1)      /* null pointer / non-positive dimension / decode workspace not 256-byte aligned */
#define TORBI_HIP_EWORKSPACE (-2)  /* workspace smaller than torbi_hip_workspace_bytes */
#define TORBI_HIP_ERANGE (-3)      /* dimension too large for this build               */
#define TORBI_HIP_ENODEVICE (-4)   /* no usable HIP device / wrong architecture        */
#define TORBI_HIP_EUNSUPPORTED (-5) /* shape not covered by this specialised entry point */

/* Build/ABI version of the loaded library (== TORBI_HIP_ABI_VERSION). */
int torbi_hip_abi_version(void);

/* Human-readable text for a return code of this library (static storage). */
const char *torbi_hip_error_string(int code);

/* Number of visible HIP devices (0 if none or the runtime failed to initialise). */
int torbi_hip_device_count(void);

/* Compute units of `device` as the tiling plans see them (256 on a whole MI355X, fewer on a
 * partitioned one); TORBI_HIP_ENODEVICE for an index that does not exist.  Queried once per device. */
int torbi_hip_compute_units(int device);

/*
 * Bytes of device scratch `torbi_hip_viterbi_decode` needs for a (B,T,S) problem.
 * Replaces the reference's internal at::zeros trellis (B,T,S) int32 + posterior (B,S)
 * fp32 allocations (viterbi.cu:331-336): the CALLER owns the scratch (e.g. a torch uint8
 * tensor from the caching allocator).  Contents need no initialisation.
 */
size_t torbi_hip_workspace_bytes(int B, int T, int S);

/*
 * Forward-recurrence paths (all give identical indices):
 *   SMALL     2 <= S <= 256: the matrix in registers for the whole decode (small_states.hpp).  Up to 64 states one
 *             wavefront per sequence, ONE launch: lane j keeps row j of the matrix, a timestep is the previous row broadcast
 *             through the LDS and S x (add, compare, max, select), byte backpointers walked back by the same wavefront
 *             (many sequences: a value-only form, the first argmax recomputed along the path).  65 .. 256 states one
 *             workgroup of ceil(S / 64)^2 waves per sequence (or per two), value-only: wave (nb, pq) keeps next-states
 *             64 nb .. x a quarter / third / half of the prev-states, the pieces of a row meet through the LDS, posterior
 *             rows go to the history and the backtrace is a launch pair of its own (speculative segments, joined
 *             exactly).  AUTO's choice up to 192 states, and up to 256 while B S^2 <= 12 * 2^16 per compute unit (larger
 *             batches: RESIDENT / CLUSTER, whose pruning then wins).  No path name: a named path that covers the shape
 *             runs instead.
 *   GENERIC   S = 1, S > 4096 with B < 32, or DENSE named for a batch below 32 items (any S): trellis kernels shaped like
 *             the reference's, one launch per timestep
 *   ROWS      B <= 16, 64 <= S <= 4096: the pruned recurrence with one wave per (item, next-state), 64 list
 *             entries per wave step (small_batch_forward.hpp); one launch per timestep.  AUTO takes it for
 *             6 .. 16 items while B S <= 12 * 1440 (beyond that one tile split over sixteen workgroups -- CLUSTER -- is
 *             faster; below six items both it and GENERIC are bound by the gap between launches)
 *   DENSE     value-only (max,+) GEMM, every (prev, next) cell evaluated, one launch per timestep
 *   (PRUNED)  the exact pruned recurrence -- sorted transition rows + per-item top posteriors bound the cells that can
 *             still win, the rest are never touched -- is what ROWS, RESIDENT and CLUSTER run.  Its one-launch-per-timestep
 *             tile form (rounds 1-3, route number 2) was removed in round 4: TORBI_HIP_FORWARD_PRUNED now names ROWS up to
 *             16 items and the time-resident forms above.
 *   RESIDENT  the pruned recurrence with the time loop inside ONE launch: a workgroup owns 16 items (8 above 2048
 *             states) x all states for every timestep, the posterior rows never leave its LDS (64 <= S <= 4096, any B).
 *             One tile per compute unit: the path for many items in flight -- several batches through
 *             torbi_hip_viterbi_decode_batches, or one batch of more than 8 * compute-units items.
 *   CLUSTER   the same kernel with each tile split over R <= 16 workgroups that scan 1/R of the next-states each and
 *             exchange their slices of every new posterior row inside the launch (self-validating 16-byte pieces: no
 *             flag, no store drain; resident_forward.hpp): the path for launches that fill at most half the compute units.  Named for a launch
 *             that fills more, it is RESIDENT.
 *   HELD      B <= 16, S <= 4096: the reference's scan with the time loop inside ONE launch: ceil(S / 8) workgroups
 *             hold 8 rows of the matrix each in registers for the whole launch and pass the posterior rows to each
 *             other through 8-byte {value, timestep} words (held_matrix_forward.hpp).
 *   BAND      (ABI 14; torbi_hip_viterbi_decode_banded only, which is told the band) a transition matrix that is -inf outside a
 *             band j - reach_left <= i <= j + reach_right -- the reference's own pitch model, torbi/evaluate/core.py:24-33 --
 *             with the time loop inside ONE launch: R workgroups share a 16-item tile, each keeps its slab of the band
 *             (diagonal-major), its window of the previous posterior row and nothing else in the LDS, evaluates every cell
 *             inside the band and none outside, and receives the hl + hr rows it needs from its two neighbours as
 *             self-validating 16-byte granules while it works on the cells that need only its own rows (band_forward.hpp).
 * AUTO: SMALL up to 64 states (up to 256 for batches that are not huge); else RESIDENT when the call's tiles fill more than half the compute units; CLUSTER for any other batch of more than
 * 16 items (64 <= S <= 4096: one batch = one forward launch); HELD up to three items (eight above 2048 states); ROWS for
 * 6..16 items (and above 2048 states); DENSE for large batches outside 64..4096 states; else GENERIC.  (The Python layer
 * adds what it knows about the matrix: DENSE for one batch with a narrow band or with scans too deep to prune.)
 *
 * A call selects a path in its `flags` (TORBI_HIP_PATH_FLAG); calls without one use the process-wide
 * default (torbi_hip_set_forward_path, initially the environment variable
 * TORBI_HIP_FORWARD=dense|pruned|resident|cluster|held, else AUTO).  A path that does not cover the shape falls
 * back as AUTO would.  A workspace of torbi_hip_workspace_bytes() fits every path.
 * torbi_hip_forward_path_on reports what a (B, S) batch would run on `device` with `flags`:
 * 0 generic, 1 dense, 3 resident, 4 rows, 5 cluster, 6 held, 7 small (2 is retired; 8 = band is reported by
 * torbi_hip_viterbi_decode_banded's phase_ms[3] and by the route record only); torbi_hip_forward_path is the same for device 0,
 * flags 0.
 */
#define TORBI_HIP_FORWARD_AUTO 0
#define TORBI_HIP_FORWARD_DENSE 1
#define TORBI_HIP_FORWARD_PRUNED 2
#define TORBI_HIP_FORWARD_RESIDENT 3
#define TORBI_HIP_FORWARD_CLUSTER 4
#define TORBI_HIP_FORWARD_HELD 5       /* B <= 16, S <= 4096: ONE launch, the matrix held in registers across the chip */
#define TORBI_HIP_FORWARD_BAND 6       /* (ABI 14) banded matrices through torbi_hip_viterbi_decode_banded; elsewhere = AUTO */
#define TORBI_HIP_PATH_FLAG(path) (((unsigned)(path) + 1u) << 4)   /* bits 4..6 of `flags`; 0 = process default */
int torbi_hip_set_forward_path(int path);
int torbi_hip_forward_path(int B, int S);
int torbi_hip_forward_path_on(int B, int S, int device, unsigned flags);
/*
 * (ABI 11) Name of the forward kernel the CALLING THREAD's most recent decode launched, spelled the way rocprofv3
 * prints kernels ("streamed::streamed_forward_kernel<15, 6>", "resident::resident_forward_kernel<12, 1, true, 1, true, 16, false>",
 * "dense::step_dense_kernel<8, 6, 8, 12, 8>", ...); empty before the first decode.  Measurement plumbing: bench.py
 * reports counter-derived figures (profiles/ *_pmc.json) only when they were taken on the kernel that is running.
 * No counterpart in the reference.
 */
int torbi_hip_last_forward_kernel(char *name_out, size_t capacity);

/*
 * The operator.  Replaces viterbi_decode_cuda (viterbi.cu:309-362) = forward trellis
 * kernel (:48-130) + argmax/repeat fill (:347-350) + backtrace kernel (:150-176).
 *
 *   observation   (B,T,S) fp32, log space          batch_frames (B) int32
 *   transition    (S,S)   fp32, [next, prev]       initial      (S) fp32
 *   indices_out   (B,T)   int32  -- fully overwritten
 *   workspace     >= torbi_hip_workspace_bytes(B,T,S) bytes, 256-byte aligned
 *
 * The decode layouts start at the caller's base, so the alignment is part of the contract of every entry point that takes
 * a decode workspace -- this one, _ex, _profiled and the torbi_hip_batch tables of _batches, _batches_prepared, _banded and
 * _banded_over: a workspace pointer that is not a multiple of 256 returns TORBI_HIP_EINVAL before any device is selected
 * and anything is launched (looked at after the size, so a workspace that is too small is TORBI_HIP_EWORKSPACE wherever it
 * lies; a batch with B == 0 brings no workspace and is not looked at).  The workspaces of the other models
 * (forward-backward, counts, k-best, sampling and their band routes) need NO alignment: those entry points round the base
 * up themselves and their size queries include the room; the streaming state needs 4 bytes (see there).
 */
int torbi_hip_viterbi_decode(const float *observation, const int32_t *batch_frames,
                             const float *transition, const float *initial,
                             int32_t *indices_out, void *workspace, size_t workspace_bytes,
                             int B, int T, int S, int device, void *stream);

/*
 * The operator with flags.  TORBI_HIP_REUSE_TRANSITION: the caller promises that the previous call
 * that used `workspace` had the same B, T, S, forward path and transition CONTENTS and that nothing
 * else has written to the workspace since; the per-transition preparation (sorted transition rows /
 * packed panels, 0.2 ms at S = 1440) is then taken from the workspace instead of being rebuilt.
 * A serving loop that decodes batch after batch with one matrix sets it from the second batch on
 * (torbi_amd.DecodePipeline does).  TORBI_HIP_PATH_FLAG(path) selects the forward path for THIS call
 * (nothing process-wide is read or written: calls from different host threads on different
 * streams/devices are independent).  flags = 0 is torbi_hip_viterbi_decode.  Unknown bits: EINVAL.
 */
#define TORBI_HIP_REUSE_TRANSITION 1u
#define TORBI_HIP_COLLECT_STATS 2u     /* accepted and ignored since round 4 (the time-resident forms always leave statistics) */
#define TORBI_HIP_SHORTEST_FIRST 256u  /* RESIDENT: workgroups in ascending order of their items' lengths (default: longest first) */
#define TORBI_HIP_FEW_SEEDS 512u       /* RESIDENT / CLUSTER: ONE explicit candidate per item (its largest posterior) instead of
                                        * three.  Same results.  For callers that have seen shallow scans with this matrix
                                        * (torbi_hip_scan_stats: ~11 of 90 list blocks per scan on the benchmark): the seed
                                        * gathers walk whole rows of the transposed matrix through the L2s -- two thirds of the
                                        * kernel's memory-side read traffic with three seeds -- and buy nothing on flat
                                        * posterior rows; on peaked rows three seeds scan a fifth fewer list blocks. */
#define TORBI_HIP_MANY_SEEDS 1024u     /* ... and THREE.  Without either flag the whole-tile form keeps three seeds and the
                                        * cluster form one (its passes run in lock step across the workgroup, so the seed
                                        * gathers' latency sits on every timestep's critical path: 512 x 1440 18.8 against
                                        * 20.7 us per timestep; peaked rows with a dense matrix are 10 % faster with three) */
int torbi_hip_viterbi_decode_ex(const float *observation, const int32_t *batch_frames,
                                const float *transition, const float *initial,
                                int32_t *indices_out, void *workspace, size_t workspace_bytes,
                                int B, int T, int S, int device, void *stream, unsigned flags);

/*
 * Several batches that share `transition`/`initial`, decoded together.  Replaces a LOOP over the
 * operator (reference torbi/core.py:417-457 decodes batch after batch): batch items are independent
 * (viterbi.cpp:65, viterbi.cu:58), so the batches of a many-file job can share one set of launches.
 * On the RESIDENT path (the AUTO choice when the group's items fill half the compute units) the whole
 * group is ONE forward launch and ONE backtrace launch; the per-transition preparation is built once,
 * in the first non-empty batch's workspace.  Otherwise the batches are decoded one after the other on
 * `stream`, each on the path it would take alone.  Every batch needs its own workspace of
 * torbi_hip_workspace_bytes(B, T, S).  Batches may differ in B and T; count <= TORBI_HIP_MAX_BATCHES.
 *
 * phase_ms: NULL, or a HOST pointer to 6 floats -- the call then brackets its phases with hipEvents on
 * `stream` and SYNCHRONISES it (bench.py):
 *   [0] forward recurrence incl. preparation, ms   [1] argmax + backtrace, ms
 *   [2] forward kernel launches                    [3] route that ran (0 generic .. 7 small)
 *   [4] per-transition preparation alone, ms       [5] batches the forward launch(es) covered
 * (for batches decoded one after the other [0],[1],[2],[4] describe the LAST batch).
 */
#define TORBI_HIP_MAX_BATCHES 16
typedef struct torbi_hip_batch {
    const float *observation;     /* (B,T,S) fp32 */
    const int32_t *batch_frames;  /* (B) int32 */
    int32_t *indices_out;         /* (B,T) int32, fully overwritten */
    void *workspace;              /* >= torbi_hip_workspace_bytes(B,T,S) bytes, 256-byte aligned */
    size_t workspace_bytes;
    int B, T;
} torbi_hip_batch;
int torbi_hip_viterbi_decode_batches(const torbi_hip_batch *batches, int count, const float *transition,
                                     const float *initial, int S, int device, void *stream, unsigned flags,
                                     float *phase_ms);

/*
 * (ABI 12) The same with the per-transition preparation of the time-resident routes (sorted and arranged transition rows,
 * transposed matrix: what TORBI_HIP_REUSE_TRANSITION is about) kept by the CALLER in `preparation`
 * (>= torbi_hip_preparation_bytes(S) bytes of device memory, 256-byte aligned; 25.6 MB at 1440 states) instead of inside the
 * first batch's workspace.  For callers that allocate scratch per call like the reference's operator does
 * (viterbi.cu:331-336): the workspace may be new every time, the preparation lives with the matrix.  With
 * TORBI_HIP_REUSE_TRANSITION the caller promises that `preparation` was filled by an earlier call with the same S and
 * transition CONTENTS on a route of the same tile size (S <= 2048 / above), ordered before this one; without the flag it
 * is (re)built.  Routes that keep no such preparation (dense, rows, generic, held) ignore the buffer AND the flag (they
 * prepare in the workspace as ever).  *filled (may be NULL) = 1 when `preparation` holds the matrix's preparation once the
 * enqueued work has run -- i.e. whether the NEXT call may pass the flag -- else 0.  preparation NULL = the plain call.
 */
size_t torbi_hip_preparation_bytes(int S);
int torbi_hip_viterbi_decode_batches_prepared(const torbi_hip_batch *batches, int count, const float *transition,
                                              const float *initial, int S, int device, void *stream, unsigned flags,
                                              float *phase_ms, void *preparation, size_t preparation_bytes, int *filled);

/*
 * (ABI 14) Banded transition matrices.  No counterpart in the reference's operator, which walks all S x S cells whatever
 * the matrix holds (viterbi.cpp:81-104, viterbi.cu:89-117); its evaluation workload is banded all the same
 * (torbi/evaluate/core.py:24-33: at most 175 finite entries per 1440-state row).
 *
 * torbi_hip_band_reach: the smallest reach_left / reach_right such that transition[j][i] == -inf whenever i < j - reach_left
 * or i > j + reach_right (-1 / -1 for a matrix without any finite entry: pass 0 / 0 on).  Runs one small kernel over the matrix on
 * `stream` and SYNCHRONISES it: call it once per matrix and keep the answer.
 *
 * torbi_hip_band_members: workgroups per 16-item tile the band kernel would use for `items` sequences with that band on
 * `device` (1 .. 16), or 0 when it does not cover the shape -- S % 4 == 0, 64 <= S <= 3072, a member's slab of the band
 * + window + merge buffer within the 160 KB LDS (at 1440 states: reach_left + reach_right <= 175 with 8 members per tile,
 * up to 16 members for fewer than 16 tiles), each reach at most a member's share of the states, reach_left + reach_right <= 508.
 *
 * (ABI 15) torbi_hip_band_members answers 1 where the band kernel runs WHOLE tiles: one workgroup per 16-item tile, the band
 * streamed from the L2 (S % 4 == 0, 64 <= S <= 1536), once the split form's launches of resident-sized pieces would add up to
 * more (8 * launches >= 5 * members; at 1440 states: from 129 tiles = 2 064 items), or for every other unit a tile where
 * the split form does not cover the band.
 *
 * torbi_hip_viterbi_decode_banded: torbi_hip_viterbi_decode_batches for a matrix whose band the caller states -- a
 * PROMISE, verified on the device (ABI 15): an entry outside the band that is not -inf is noticed by the launch that looks
 * at the matrix, and every item is then decoded again on the whole matrix (slow, identical to the reference).  Same arguments,
 * same workspaces (torbi_hip_workspace_bytes covers the route), same phase_ms (phase_ms[3] = 8 when the band kernel ran).
 * `transition` and the observations must be 16-byte aligned for the band kernel.  The band kernel runs for TORBI_HIP_FORWARD_AUTO and
 * TORBI_HIP_FORWARD_BAND when its plan covers the group -- under AUTO except for shapes SMALL decodes and for the handful
 * of sequences HELD takes --; otherwise, and for every other named path, the call IS torbi_hip_viterbi_decode_batches
 * (BAND named: as AUTO).  Waits inside the launch are bounded and repaired as in the CLUSTER form (give-ups are counted
 * in torbi_hip_scan_stats [127]; TORBI_HIP_CLUSTER_WAIT_US overrides the budget).
 */
int torbi_hip_band_reach(const float *transition, int S, int device, void *stream, int *reach_left_out, int *reach_right_out);
int torbi_hip_band_members(int items, int S, int reach_left, int reach_right, int device);
int torbi_hip_viterbi_decode_banded(const torbi_hip_batch *batches, int count, const float *transition, const float *initial,
                                    int S, int reach_left, int reach_right, int device, void *stream, unsigned flags,
                                    float *phase_ms);

/*
 * (ABI 15) A band with ONE CONSTANT outside it.  The reference's evaluation does not decode with log(p) but with
 * log(p + tiny) (torbi/evaluate/core.py:97-103 -> torbi/core.py:341-347): its pitch matrix holds log(tiny) = -87.34 outside the
 * band, not -inf, and candidates from out there do win on rows whose posteriors fall that far.  Every such candidate is
 * fl(post[i] + c), so the best of them is fl(M + c), M the largest posterior outside the band (rounding is monotone): the
 * whole-tile band kernel keeps every row's maximum and where it is attained, and decides every output exactly
 * (csrc/band_tile_forward.hpp; what it cannot decide -- in-band entries BELOW the constant where the row's maximum stands --
 * is decoded again in the reference's order).  The `_over` entry points are the banded ones with `background` = that constant
 * (-inf: identical to them): torbi_hip_band_reach_over takes the matrix's corner entry transition[0][S - 1] for it (bit for
 * bit) and answers the reach over every other value -- S - 1 / S - 1 ("no band") for a finite constant unless every other
 * entry lies ABOVE it, as in a pitch matrix: where the band reaches down to the constant, outputs next to a row's maximum
 * cannot be decided from the maximum alone and the batch would be decoded again every time; torbi_hip_band_members_over answers like torbi_hip_band_members (the split
 * form exchanges its members' row maxima: csrc/band_forward.hpp, band_forward_kernel<true>).
 */
int torbi_hip_band_reach_over(const float *transition, int S, int device, void *stream, int *reach_left_out, int *reach_right_out,
                              float *background_out);
int torbi_hip_band_members_over(int items, int S, int reach_left, int reach_right, float background, int device);
int torbi_hip_viterbi_decode_banded_over(const torbi_hip_batch *batches, int count, const float *transition, const float *initial,
                                         int S, int reach_left, int reach_right, float background, int device, void *stream,
                                         unsigned flags, float *phase_ms);

/*
 * Scan statistics for adaptive path selection (torbi_amd/viterbi.py uses them): copies 128 uint32 to `stats_out`
 * (DEVICE pointer) on `stream`.  Which of the two records below is copied is decided ON THE DEVICE by the route the last
 * decode with `workspace` actually took (every decode stamps it behind its scratch layout: a batch decoded inside a
 * launch group takes the group's route, whatever its own shape and flags would have chosen); `flags` is accepted for
 * compatibility and ignored.  Zeros for a decode on another route.
 *   RESIDENT (always collected; `workspace` = the FIRST batch's workspace of the launch group):
 *     stats_out[0]       list blocks walked by the sampled wave passes (every 16th timestep)
 *     stats_out[64]      wave passes counted
 *     stats_out[127]     (CLUSTER) workgroups that gave up waiting for their cluster; 0 on any sane run
 *   RESIDENT / CLUSTER / BAND / DENSE (ABI 14): stats_out[120], [121] = shader-clock ticks and 100 MHz wall-clock ticks of the
 *                        forward kernel's workgroup 0 (same unit both; DENSE: of the last timestep's launch) -- their ratio
 *                        x 100 MHz is the clock the kernel was delivered under its own load (measurement plumbing: bench.py
 *                        prices the vector ALU's ceiling at it)
 *   RESIDENT / CLUSTER / BAND, one batch of at most 1024 sequences: stats_out[122], [123] = path steps of the backtrace and
 *                        steps walked AGAIN where its speculative segments met (csrc/lazy_backtrace.hpp, chase_segment)
 *   BAND: stats_out[127] = members that gave up waiting (as CLUSTER)
 *   HELD: stats_out[127] = workgroups that ran out of polls (the launch could not be resident as a whole); the decode
 *                        was then redone by the repair kernel and its results are correct.  0 on any sane run.
 * sum(first half) / sum(second half) = list blocks per scan: about 11 of the S/16 = 90 on the 1440-state benchmark;
 * near S/16 nothing is being pruned and the dense path is faster.  TORBI_HIP_EUNSUPPORTED when the shape takes
 * neither path.
 */
int torbi_hip_scan_stats(const void *workspace, size_t workspace_bytes, int B, int T, int S,
                         unsigned *stats_out, int device, void *stream, unsigned flags);

/*
 * The operator for a UNIFORM transition matrix (every entry == log_transition), i.e. the
 * reference's default when from_probabilities() is called without a transition
 * (torbi/core.py:175-180 builds torch.full((S,S), log(1/S)) and runs the generic recurrence).
 * With identical rows the backpointer is the same for every next state, so the decode is O(S)
 * per timestep, needs no scratch and streams the observations once (HBM-bound).  Results are
 * bit-identical to torbi_hip_viterbi_decode on the materialised matrix.
 * Covers S % 4 == 0, S <= 4096, 16-byte aligned observation/initial; otherwise returns
 * TORBI_HIP_EUNSUPPORTED and the caller materialises the matrix.
 */
int torbi_hip_viterbi_decode_uniform(const float *observation, const int32_t *batch_frames,
                                     float log_transition, const float *initial,
                                     int32_t *indices_out, int B, int T, int S, int device,
                                     void *stream);
/*
 * (ABI 13) The same with the observations given as PROBABILITIES, the way from_probabilities() receives them by default
 * (log_probs=False): every element goes through the reference's torch.log and the epsilon round trip log(exp(x) + tiny)
 * (torbi/core.py:189-197; bit-identical to torbi_hip_log_epsilon_clamp, i.e. to the torch ops) as it is read, so the whole
 * default call -- probabilities in, no transition given -- is ONE pass over the observations.  `probabilities` is not
 * written (upstream's torch.log is out of place too).  `initial` is in log space as before.
 */
int torbi_hip_viterbi_decode_uniform_probabilities(const float *probabilities, const int32_t *batch_frames,
                                                   float log_transition, const float *initial, int32_t *indices_out,
                                                   int B, int T, int S, int device, void *stream);

/*
 * Same operator, instrumented for bench.py: torbi_hip_viterbi_decode_batches for one batch with
 * `phase_ms` (a HOST pointer to 6 floats, see there); SYNCHRONISES the stream.
 */
int torbi_hip_viterbi_decode_profiled(const float *observation, const int32_t *batch_frames,
                                      const float *transition, const float *initial,
                                      int32_t *indices_out, void *workspace,
                                      size_t workspace_bytes, int B, int T, int S, int device,
                                      void *stream, unsigned flags, float *phase_ms);

/*
 * Test/diagnostic access to the final posterior rows the forward pass produced by the last
 * decode that used `workspace` (reference: the `posterior` tensor, viterbi.cu:334-336).
 * Copies (B,S) fp32 into `posterior_out` (device pointer) on `stream`.  Where the rows live depends on the route that
 * decode took; it is read on the device from the route record the decode left in the workspace (`flags` is accepted for
 * compatibility and ignored).
 */
int torbi_hip_read_posterior(const void *workspace, size_t workspace_bytes,
                             const int32_t *batch_frames, float *posterior_out,
                             int B, int T, int S, int device, void *stream, unsigned flags);

/*
 * In-place epsilon clamp of from_probabilities (reference torbi/core.py:193-197):
 *     x <- log(exp(x) + FLT_MIN)        three torch ops upstream (exp_, += tiny, log_)
 * fused into one pass over the (B,T,S) observation tensor.  Uses the same device math
 * functions as PyTorch-ROCm's elementwise kernels; tests/test_gpu_parity.py checks bit
 * equality with the three torch ops on the same device.
 */
int torbi_hip_epsilon_clamp(float *x, uint64_t count, int device, void *stream);

/*
 * The same for PROBABILITY inputs: out <- log(exp(log(p)) + FLT_MIN), i.e. upstream's torch.log(observation)
 * (torbi/core.py:189-191, out of place) and the clamp behind it in one pass instead of four.  `probabilities`
 * is not written unless `out` == `probabilities` (in place: the many-file driver's own copies of its files); both
 * pointers 16-byte aligned.
 */
int torbi_hip_log_epsilon_clamp(const float *probabilities, float *out, uint64_t count, int device, void *stream);

/*
 * Measurement helper (not part of the reference interface): fills dst[0..count) with the
 * deterministic synthetic scores of torbi_amd/synth.py -- value(k) = 0 - u24(hash(stream_id,
 * seed, start + k)) * 2^-20 -- so bench.py can build the 1.5 GB headline input in HBM
 * without a host round trip.  Bit-identical to the numpy definition (tested).
 */
int torbi_hip_fill_synthetic(float *dst, uint64_t count, uint64_t start, int stream_id,
                             int seed, int device, void *stream);

/*
 * (ABI 14) The host side of a many-file job -- reading the payloads of torch.save()d observations into a batch buffer,
 * writing the decoded sequences' files, opening a batch of files -- lives in libtorbi_cpu.so ALONE (include/torbi_cpu.h:
 * torbi_cpu_read_rows, torbi_cpu_write_files, torbi_cpu_open_heads).  Rounds 2-4 exported the same functions from this
 * library as torbi_hip_read_rows / _write_files / _open_heads; they touch no device, and their first call from a reader thread
 * used to wait behind the HIP runtime's start-up on the calling thread (0.35-0.65 s per early batch of a cold job).
 */

/*
 * (ABI 16) Streaming decode: B independent streams, frames pushed in pieces, the indices of every frame returned as soon
 * as no later frame can change them (torbi_amd/stream.py, STREAM.md).  Frame c of a stream is DECIDED once the
 * survivor paths of ALL S states at the newest frame pass through one state at c; a push returns the frames up to the
 * newest decided one, a flush the rest.  Concatenated, they are bit-identical to torbi_hip_viterbi_decode on the whole
 * sequence (result contract above, NaN / +-inf included).
 *
 * State (caller-owned, device memory, torbi_hip_stream_state_bytes(B, S, capacity) bytes, no alignment beyond 4):
 *     ring  [B][capacity][S] fp32   posterior rows of the pending frames (frame base + r in slot (base_slot + r) % capacity)
 *     memo  [B][capacity]    int32  survivor-set sizes of earlier frontier walks (need no initialisation)
 *     bp    [B][S]           int32  scratch
 * Only the ring has to be kept when the state grows: a larger state takes the pending rows (and the newest row) in their
 * new slots and a zeroed memo.  capacity >= pending + frames of every stream of a push, >= 1.
 *
 * info: [B][4] int32 device array per call: {pending, base_slot, frames, fresh}.  `pending` frames pushed and not yet
 * returned, `base_slot` the slot of the first of them, `frames` (push: 0 .. Tc new frames of this stream; flush: 1 = flush
 * this stream, 0 = leave it), `fresh` = 1 when the stream has no frame yet (its first row is obs[0] + initial).
 *
 * push: observation (B, Tc, S) (Tc may be 0); transition (S, S) [next][prev] and transition_t, the same matrix transposed
 * ([prev][next]); initial (S,).  indices_out [B][out_capacity] int32 (out_capacity >= pending + frames): row b receives the
 * stream's newly decided frames, oldest first; counts_out [B] int32 their number.  The caller advances base_slot by
 * counts_out[b] and pending by frames - counts_out[b].
 * counts_out[b] = -1 (checked by every kernel of the call, not only the last): the stream's info does not fit --
 * pending < 0, base_slot outside 0 .. capacity - 1, frames outside 0 .. Tc (push), or pending + frames above capacity or
 * out_capacity -- and the stream's ring, memo and indices_out row are untouched; the other streams of the call are decoded.
 * flush: the flagged streams' remaining frames (the final state is the first NaN of the newest row, otherwise its first
 * maximum), counts_out as above; the caller then starts those streams afresh.
 * TORBI_HIP_ERANGE for S > 8000.
 *
 * torbi_hip_stream_tile (added within ABI 17) reports how many streams share one workgroup of a push's forward kernel for a (B, S) call
 * on `device`: 1, 2, 4, 8 or 16 (stream_forward_kernel<G, J> of csrc/stream.hpp; J = 4 where S % 4 == 0 and transition_t is
 * 16-byte aligned, else 1), a function of (B, S, compute units) only and the choice the push itself makes; TORBI_HIP_EINVAL /
 * TORBI_HIP_ERANGE for a shape the push turns down.  Touches no device memory; without a usable device it answers for 256
 * compute units.
 *
 * torbi_hip_stream_push_lag (added within ABI 17) is the push with a decision depth (truncated, or fixed-lag, Viterbi): at
 * most `max_lag` frames of a stream stay pending after the call.  With n frames so far and c_nat the newest frame the rule
 * above decides (-1: none), a stream that receives at least one frame returns its frames up to c = max(c_nat, n - 1 - max_lag).
 * Frames above c_nat are FORCED: their states lie on the backtrace from the final state of the newest row (its first NaN,
 * otherwise its first maximum: flush's rule), so every call's output is the corresponding span of the whole-sequence decode
 * of the stream's first n frames.  A forced span and the span after it need not join into one path: a later frame may move
 * the best path, nothing is repaired.  forced_out [B] int32: how many of the counts_out[b] frames were forced (0 for a
 * stream whose info does not fit, or that received no frame); state, info, indices_out and counts_out as for the push.
 * max_lag = -1: no bound, forced_out may be NULL and the call IS torbi_hip_stream_push (which forwards here).
 * TORBI_HIP_EINVAL for max_lag < -1 and for max_lag >= 0 without forced_out, looked at after every argument of the push.
 * With pending <= max_lag the caller's ring never needs more than max_lag + Tc slots.
 */
size_t torbi_hip_stream_state_bytes(int B, int S, int capacity);
int torbi_hip_stream_push(const float *observation, int Tc, const int32_t *info, const float *transition,
                          const float *transition_t, const float *initial, void *state, size_t state_bytes, int capacity,
                          int32_t *indices_out, int out_capacity, int32_t *counts_out, int B, int S, int device, void *stream);
int torbi_hip_stream_push_lag(const float *observation, int Tc, const int32_t *info, const float *transition,
                              const float *transition_t, const float *initial, void *state, size_t state_bytes, int capacity,
                              int32_t *indices_out, int out_capacity, int32_t *counts_out, int max_lag, int32_t *forced_out,
                              int B, int S, int device, void *stream);
int torbi_hip_stream_flush(const int32_t *info, const float *transition, void *state, size_t state_bytes, int capacity,
                           int32_t *indices_out, int out_capacity, int32_t *counts_out, int B, int S, int device, void *stream);
int torbi_hip_stream_tile(int B, int S, int device);

/*
 * (added within ABI 17) The band route of streaming decode: the decoder above, bit for bit (NaN, +-inf and ties included),
 * for a transition matrix that holds ONE value outside a band -- transition[j][i] == background (bit for bit) unless
 * j - reach_left <= i <= j + reach_right -- at the cost of the band: W = reach_left + reach_right + 1 candidates per state
 * and frame plus two scans of the previous row for the candidates outside it (csrc/stream_band.hpp, STREAM.md "Band
 * route").  The forward keeps each frame's backpointers, so the frontier walk, the forced frames of a decision depth and
 * the backtrace follow stored pointers and read neither scores nor the matrix: a push is two launches, a flush one.
 *
 * State: the same torbi_hip_stream_state_bytes(B, S, capacity) bytes, laid out
 *     ring    [B][capacity][S] int32  backpointers of the pending frames (frame base + r in slot (base_slot + r) % capacity;
 *                                     the row of the first pending frame is never read)
 *     memo    [B][capacity]    int32  as above
 *     carried [B][S]           fp32   the newest posterior row
 * A state that grows takes the pointer rows of the pending frames in their new slots, the carried rows and a zeroed memo.
 * A state belongs to ONE route: the two layouts are not interchangeable.
 *
 * torbi_hip_stream_band_covers answers 1 where the route takes a call, else 0, without touching a device: S % 4 == 0,
 * 64 <= S <= 3072, reach_left, reach_right >= 0, reach_left + reach_right + 4 <= 512 (what torbi_hip_band_reach_over's
 * callers can be told about a matrix; the rows with their halos and the scans of one stream,
 * (6 S + 2 (reach_left + reach_right)) * 4 bytes, then fit the 160 KB of LDS with room to spare) and a background that is
 * neither NaN nor +inf (-inf and every finite value are taken by the same kernels).
 * torbi_hip_stream_band_tile reports how many streams share one workgroup of a push's forward kernel
 * (stream_band_forward_kernel<G>: 1, 2 or 4 -- the largest whose LDS, (6 S + 2 (reach_left + reach_right)) * 4 G bytes, fits
 * 159 KB, halved while there are fewer workgroups than compute units); the choice the push itself makes.  EINVAL /
 * EUNSUPPORTED for a shape the push turns down; without a usable device it answers for 256 compute units.
 *
 * torbi_hip_stream_band_prepare, once per matrix: diagonals_out [W][S] fp32 (torbi_hip_stream_band_diagonals_bytes; 0 for an
 * argument < 0) receives diag[k][j] = transition[j][j - reach_left + k], and ok_out[0] (int32, device) 1 where every entry
 * outside the band equals `background` bit for bit, else 0: the caller reads it before it trusts the diagonals.
 *
 * torbi_hip_stream_band_push: torbi_hip_stream_push_lag with `diagonals` in place of the two matrices (max_lag = -1: no
 * bound, forced_out may be NULL); info, indices_out, counts_out (-1: info does not fit, the stream's state and output row
 * untouched), forced_out and the argument rules as there -- EINVAL, ERANGE (S > 8000), EWORKSPACE, then the entry's own:
 * EINVAL for a negative reach, EUNSUPPORTED where _covers answers 0.  torbi_hip_stream_band_flush: torbi_hip_stream_flush
 * on such a state (EUNSUPPORTED for an S the route does not take).  Every argument is checked before any device work.
 */
int torbi_hip_stream_band_covers(int B, int S, int reach_left, int reach_right, float background, int device);
int torbi_hip_stream_band_tile(int B, int S, int reach_left, int reach_right, int device);
size_t torbi_hip_stream_band_diagonals_bytes(int S, int reach_left, int reach_right);
int torbi_hip_stream_band_prepare(const float *transition, int S, int reach_left, int reach_right, float background,
                                  float *diagonals_out, int32_t *ok_out, int device, void *stream);
int torbi_hip_stream_band_push(const float *observation, int Tc, const int32_t *info, const float *diagonals, const float *initial,
                               int reach_left, int reach_right, float background, void *state, size_t state_bytes, int capacity,
                               int32_t *indices_out, int out_capacity, int32_t *counts_out, int max_lag, int32_t *forced_out,
                               int B, int S, int device, void *stream);
int torbi_hip_stream_band_flush(const int32_t *info, void *state, size_t state_bytes, int capacity, int32_t *indices_out,
                                int out_capacity, int32_t *counts_out, int B, int S, int device, void *stream);

/*
 * (added within ABI 17) Streaming posteriors: online filtering and fixed-lag smoothing of B independent streams whose
 * frames arrive in pieces (csrc/stream_posterior.hpp, torbi_amd/stream_posterior.py, STREAM.md "Streaming posteriors").  The
 * quantities are torbi_hip_forward_backward's (the scaled recurrence of POSTERIOR.md, its non-finite rules included).  A
 * stream holds n frames, the first `base` of them returned; a push of f >= 1 frames returns, with n' = n + f, the rows
 * gamma_{t|n'} = P(state_t | frames 0 .. n' - 1) for t = base .. n' - 1 - lag: the corresponding rows of the whole-sequence
 * posteriors of the stream's first n' frames.  A stream with f = 0 returns nothing and keeps its state.  A flush returns the
 * rows base .. n - 1 as gamma_{t|n}.  A stream whose running log-likelihood is not finite returns NaN rows.
 *
 * expa (S, S) fp32 is exp(transition) [next][prev] and expa_t the same matrix transposed ([prev][next]); the caller builds
 * both once per matrix (there is no prepare kernel; torbi_amd builds them with torch.exp from a private copy).  Where
 * S % 4 == 0 and the matrix a kernel reads is 16-byte aligned, a thread takes 4 consecutive states per 16-byte load.
 *
 * State (caller-owned, device memory, torbi_hip_stream_posterior_state_size(B, S, capacity) bytes -- 0 for a non-positive
 * argument --, no alignment beyond 4, no initialisation: the `fresh` flag is what starts a stream), 4-byte words, packed:
 *     L  [B][2]           the fp64 running sum of log c_t + m_t, low word first; log P(frames so far) of a started stream
 *     a  [B][capacity][S] fp32   a_t of the pending frames (frame base + r in slot (base_slot + r) % capacity)
 *     e  [B][capacity][S] fp32   e_t
 *     c  [B][capacity]    fp32   c_t
 *     m  [B][capacity]    fp32   m_t
 * The newest frame's a and c are read by the next push in the slot before the first free one, also when nothing is
 * pending.  A state that grows takes L and the rows of the pending frames and of the newest frame in their new slots.
 * capacity >= pending + frames of every stream of a push, >= 1; with pending <= lag it never needs more than lag + Tc.
 *
 * info [B][4] int32 {pending, base_slot, frames, fresh} as for torbi_hip_stream_push (flush: frames = 1 flushes the stream,
 * 0 leaves it).  posterior_out [B][out_capacity][S] fp32: row r of stream b is its frame base + r; counts_out [B] int32
 * (may be NULL) the number of rows, -1 for a stream whose info does not fit -- pending < 0 or above capacity, base_slot
 * outside 0 .. capacity - 1, fresh with pending != 0, frames outside 0 .. Tc or above capacity - pending, or more rows to
 * return than out_capacity.  One predicate decides this in every kernel of the call: such a stream keeps its state and its
 * output rows untouched, the others are processed.  The caller advances base_slot by the count and sets pending to
 * pending + frames - count.  Neither call synchronises the host or reads anything back.
 *
 * torbi_hip_stream_posterior_tile: streams per workgroup of a call's kernels for (B, S) on `device` (sp_forward_kernel<G, J>
 * and sp_backward_kernel<G, J>: 16, halved while the rows of G streams, 8 G S bytes, and 768 bytes of partial sums exceed
 * 64 KB of LDS, then while there are fewer workgroups than compute units); EINVAL / ERANGE for a shape the push turns down;
 * without a usable device it answers for 256 compute units.
 *
 * Every argument is checked before any device work: TORBI_HIP_EINVAL (a null pointer -- counts_out may always be null,
 * observation / expa_t / initial when Tc = 0 --; B, S, capacity or out_capacity < 1; Tc < 0; lag < 0), TORBI_HIP_ERANGE for
 * S > 8000 (the double-buffered rows of one stream in 64 KB of LDS), TORBI_HIP_EWORKSPACE for a state_bytes below the size.
 */
size_t torbi_hip_stream_posterior_state_size(int B, int S, int capacity);
int torbi_hip_stream_posterior_tile(int B, int S, int device);
int torbi_hip_stream_posterior_push(const float *observation, int Tc, const int32_t *info, const float *expa, const float *expa_t,
                                    const float *initial, void *state, size_t state_bytes, int capacity, float *posterior_out,
                                    int out_capacity, int32_t *counts_out, int lag, int B, int S, int device, void *stream);
int torbi_hip_stream_posterior_flush(const int32_t *info, const float *expa, void *state, size_t state_bytes, int capacity,
                                     float *posterior_out, int out_capacity, int32_t *counts_out, int B, int S, int device,
                                     void *stream);

/*
 * (added within ABI 17) The band route of streaming posteriors, for a transition matrix that holds ONE value outside a band
 * (csrc/stream_posterior_band.hpp, STREAM.md "Streaming posteriors: band route"): what torbi_hip_stream_posterior_push and
 * torbi_hip_stream_posterior_flush compute, their info, outputs, counts_out and non-finite rules, on a state of the same
 * layout and size (torbi_hip_stream_posterior_state_size; a state may change routes between two calls), at the cost of the
 * band: W = reach_left + reach_right + 1 multiplies per state and step where the dense route spends S.  The caller states
 * the band j - reach_left <= i <= j + reach_right of transition [next j][prev i] (log scores) and `background`, the value
 * of every entry outside it.  The bits differ from the dense route's; a stream's bits depend on its own data and on
 * (t, n') only, as there.
 *
 * torbi_hip_stream_smooth_band_covers answers 1 where the route takes a call, else 0, without touching a device: B >= 1,
 * 1 <= S <= 4096 (odd S and unaligned rows included), reach_left, reach_right >= 0 with min(W, S) <= 64 after the reaches
 * are clamped to S - 1, and a background that is neither NaN nor +inf (-inf and every finite value are taken by the same
 * kernels): what torbi_hip_forward_backward_band_covers takes of a matrix.
 * torbi_hip_stream_smooth_band_tile: streams per workgroup of a call's kernels (spb_forward_kernel<G> and
 * spb_backward_kernel<G>: 8, halved while the rows of G streams with their halos and wave sums,
 * 8 G (S + 2 max(reach_left, reach_right) + 16) bytes, exceed 64 KB of LDS, then while there are fewer workgroups than compute
 * units); EINVAL / EUNSUPPORTED for a shape the push turns down; without a usable device it answers for 256 compute units.
 *
 * torbi_hip_stream_smooth_band_prepare, once per matrix: diagonals_out (torbi_hip_stream_smooth_band_diagonals_size bytes,
 * 2 W roundup(S, 64) floats; 0 for S < 1 or a negative reach) receives the diagonals of exp(transition) - exp(background)
 * along the next state and along the prev state, 0 where the matrix edge clips one, and ok_out[0] (int32, device) 1 where
 * every entry outside the band equals `background` bit for bit, else 0: the caller reads it before it trusts the diagonals.
 *
 * push and flush: the dense calls with `diagonals`, reach_left, reach_right and background in place of expa / expa_t.
 * Every argument is checked before any device work: the dense entries' codes as they stand (EINVAL, ERANGE, EWORKSPACE),
 * then EINVAL for a negative reach and EUNSUPPORTED where _covers answers 0.  Neither call synchronises the host.
 */
int torbi_hip_stream_smooth_band_covers(int B, int S, int reach_left, int reach_right, float background, int device);
int torbi_hip_stream_smooth_band_tile(int B, int S, int reach_left, int reach_right, int device);
size_t torbi_hip_stream_smooth_band_diagonals_size(int S, int reach_left, int reach_right);
int torbi_hip_stream_smooth_band_prepare(const float *transition, int S, int reach_left, int reach_right, float background,
                                         float *diagonals_out, int32_t *ok_out, int device, void *stream);
int torbi_hip_stream_smooth_band_push(const float *observation, int Tc, const int32_t *info, const float *diagonals, int reach_left,
                                      int reach_right, float background, const float *initial, void *state, size_t state_bytes,
                                      int capacity, float *posterior_out, int out_capacity, int32_t *counts_out, int lag, int B,
                                      int S, int device, void *stream);
int torbi_hip_stream_smooth_band_flush(const int32_t *info, const float *diagonals, int reach_left, int reach_right,
                                       float background, void *state, size_t state_bytes, int capacity, float *posterior_out,
                                       int out_capacity, int32_t *counts_out, int B, int S, int device, void *stream);

/*
 * (ABI 17) Forward-backward: per-frame state posteriors and the sequence log-likelihood of the HMM that
 * torbi_hip_viterbi_decode decodes (torbi_amd/posterior.py, POSTERIOR.md).  Inputs as there: observation (B, T, S) log
 * scores, batch_frames (B,) int32 (clamped to [1, T]), transition (S, S) log [next][prev], initial (S,) log.  For t < F_b:
 *     log alpha_0[j] = initial[j] + obs_0[j],  log alpha_t[j] = obs_t[j] + logsumexp_i (transition[j][i] + log alpha_{t-1}[i])
 *     log beta_{F-1}[j] = 0,                   log beta_t[i]  = logsumexp_j (transition[j][i] + obs_{t+1}[j] + log beta_{t+1}[j])
 *     L_b = logsumexp_j log alpha_{F-1}[j],    gamma_t[j]     = exp(log alpha_t[j] + log beta_t[j] - L_b)
 * posterior_out (B, T, S) fp32 receives gamma (rows t >= F_b are 0), loglik_out (B,) fp32 receives L (summed in fp64).
 * -inf entries are zero probabilities.  An item of total probability 0 gets L = -inf and NaN rows t < F_b; a NaN or +inf in
 * anything an item reads gives it L = NaN and NaN rows; an item's bits never depend on other items' data.
 *
 * workspace: device scratch of torbi_hip_forward_backward_workspace_bytes(B, T, S) bytes (no initialisation, no
 * alignment: the call rounds the base up to 256 bytes itself and the size includes the room; both entry points).  What the
 * workspace held before never reaches a result.  One launch per timestep and pass, no host synchronisation: a call can be
 * captured into a graph.
 * The uniform entry point takes a matrix whose every entry is `uniform_value` (torbi_amd passes fl(log(1/S))) and computes
 * the same quantities in closed form (beta is constant over states): one elementwise pass and a per-item fp64 sum.
 * TORBI_HIP_ERANGE for S > 16384, more than 65535 * 32 items or more than 2^32 item frames (B * T).
 */
size_t torbi_hip_forward_backward_workspace_bytes(int B, int T, int S);
int torbi_hip_forward_backward(const float *observation, const int32_t *batch_frames, const float *transition,
                               const float *initial, float *posterior_out, float *loglik_out, void *workspace,
                               size_t workspace_bytes, int B, int T, int S, int device, void *stream);
int torbi_hip_forward_backward_uniform(const float *observation, const int32_t *batch_frames, float uniform_value,
                                       const float *initial, float *posterior_out, float *loglik_out, void *workspace,
                                       size_t workspace_bytes, int B, int T, int S, int device, void *stream);

/*
 * Expected counts (added within ABI 17): torbi_hip_forward_backward on the same inputs, which writes posterior_out and
 * loglik_out bit for bit as that call does, and in addition, with a per-item weight g_b (item_weights (B,) fp32; null:
 * all ones) and xi_t(j, i) = P(s_{t-1} = i, s_t = j | obs_b):
 *     counts_out[j][i]      = sum_b g_b sum_{1 <= t < F_b} xi_t(j, i)      (S, S) fp32, [next][prev] like `transition`
 *     initial_counts_out[j] = sum_b g_b gamma_0^b[j]                        (S,) fp32
 * An item with g_b == 0 or a non-finite L_b is skipped, not multiplied: a NaN item adds nothing.  The summation order is
 * fixed (over t from F - 1 down to 1, over items in order), so the bits of both outputs depend on the inputs only; no
 * float atomics.  workspace: torbi_hip_forward_backward_counts_workspace_bytes(B, T, S) bytes, no alignment.  No host
 * synchronisation: with a caller-owned workspace a call can be captured into a graph.  Errors as torbi_hip_forward_backward, and
 * TORBI_HIP_EINVAL for a null counts_out or initial_counts_out.
 */
size_t torbi_hip_forward_backward_counts_workspace_bytes(int B, int T, int S);
int torbi_hip_forward_backward_counts(const float *observation, const int32_t *batch_frames, const float *transition,
                                      const float *initial, const float *item_weights, float *posterior_out,
                                      float *loglik_out, float *counts_out, float *initial_counts_out, void *workspace,
                                      size_t workspace_bytes, int B, int T, int S, int device, void *stream);

/*
 * Band route of forward-backward (added within ABI 17): torbi_hip_forward_backward's quantities for a matrix that holds ONE
 * value outside a band.  The caller states the band -- transition[j][i] with j - reach_left <= i <= j + reach_right ([next][prev],
 * as torbi_hip_band_reach_over answers) -- and `background` (finite or -inf), and promises that every entry outside the band
 * equals `background` bit for bit.  With ebg = exp(background) (0 for -inf) each product is the band's sum of
 * (exp(transition) - ebg) plus ebg times the operand's sum, so a frame costs W = reach_left + reach_right + 1 multiplies per
 * state.  The call reads the whole matrix once on the device and checks the promise: where it is broken, every log-likelihood
 * and every posterior row t < F_b is NaN (no error code: nothing waits for the device).  Contract, non-finite rules and
 * independence of items as torbi_hip_forward_backward (an in-band NaN or +inf reaches every item with F_b >= 2); the
 * rounding differs from the dense route's, an item's bits do not depend on how many items share its workgroup.
 *
 * torbi_hip_forward_backward_band_covers: 1 where the entry point takes the call -- 1 <= S <= 4096, at most 64 in-band
 * entries in a matrix row (min(W, S) <= 64 with the reaches clamped to S - 1), a background that is neither NaN nor +inf, B
 * and T within torbi_hip_forward_backward's limits --, else 0.  It and _workspace_bytes answer without a device.
 * workspace: torbi_hip_forward_backward_band_workspace_bytes(B, T, S, reach_left, reach_right) bytes, no initialisation (the
 * promise flag is reset by every call) and no alignment.
 * Four launches per call whatever T is (the time loop runs inside one launch, a workgroup owns whole items), no host
 * synchronisation: with a caller-owned workspace a call can be captured into a graph.  Errors as
 * torbi_hip_forward_backward (TORBI_HIP_EINVAL also for a negative reach), and TORBI_HIP_EUNSUPPORTED where _covers answers 0.
 */
int torbi_hip_forward_backward_band_covers(int B, int T, int S, int reach_left, int reach_right, float background, int device);
size_t torbi_hip_forward_backward_band_workspace_bytes(int B, int T, int S, int reach_left, int reach_right);
int torbi_hip_forward_backward_band(const float *observation, const int32_t *batch_frames, const float *transition,
                                    const float *initial, int reach_left, int reach_right, float background,
                                    float *posterior_out, float *loglik_out, void *workspace, size_t workspace_bytes, int B,
                                    int T, int S, int device, void *stream);

/*
 * Expected counts on a band (added within ABI 17): torbi_hip_forward_backward_band on the same inputs, which writes
 * posterior_out and loglik_out bit for bit as that call does, and in addition the counts of
 * torbi_hip_forward_backward_counts inside the band, diagonal by diagonal, and the initial counts:
 *     band_counts_out[k][j] = X[j][j - reach_left + k]      (W, S) fp32, W = reach_left + reach_right + 1 with the reaches
 *                                                            clamped to S - 1; 0 where the matrix clips the diagonal
 *     initial_counts_out[j] = sum_b g_b gamma_0^b[j]        (S,) fp32
 * with X[j][i] = sum_b g_b sum_{1 <= t < F_b} xi_t(j, i), item_weights (B,) fp32 (null: all ones).  An item with g_b == 0 or a
 * non-finite L_b is skipped, not multiplied.  The counts are gathered inside the backward pass of the one launch that runs
 * all frames (one fp32 plane [W][S] in LDS per workgroup, at most 512 workgroups, each over its tiles in order) and summed
 * over the workgroups in order: the summation order is fixed, so the bits depend on the inputs (and the device's compute
 * unit count, which sets the tile) only; no float atomics.  Where the promise about the band is broken, every entry of both
 * outputs is NaN as well.
 *
 * A finite background puts mass outside the band: X[j][i] = exp(background) * sum_b g_b sum_t w_t[j] a_{t-1}[i] / c_{t-1}
 * there.  That is a dense product of rank sum_b F_b and is NOT computed: the call returns the in-band counts only.  The
 * total outside the band is sum_b g_b (F_b - 1) over the counted items minus the band's total.
 *
 * torbi_hip_forward_backward_counts_band_covers: 1 where torbi_hip_forward_backward_band_covers answers 1 AND the plane fits
 * beside the rows of one item, 4 W S + the rows' bytes <= 160 KB (the pitch band, 23 diagonals of 1440 states: 144 KB), else
 * 0.  It and _workspace_bytes answer without a device.  workspace: the band route's plus min(B, 512) planes [W][S up to 64]
 * fp32, torbi_hip_forward_backward_counts_band_workspace_bytes(B, T, S, reach_left, reach_right) bytes, no initialisation
 * and no alignment.
 * Six launches per call whatever T is, no host synchronisation: with a caller-owned workspace a call can be captured into a
 * graph.  Errors as torbi_hip_forward_backward_band, TORBI_HIP_EINVAL also for a null band_counts_out or
 * initial_counts_out, TORBI_HIP_EUNSUPPORTED where _covers answers 0.
 */
int torbi_hip_forward_backward_counts_band_covers(int B, int T, int S, int reach_left, int reach_right, float background,
                                                  int device);
size_t torbi_hip_forward_backward_counts_band_workspace_bytes(int B, int T, int S, int reach_left, int reach_right);
int torbi_hip_forward_backward_counts_band(const float *observation, const int32_t *batch_frames, const float *transition,
                                           const float *initial, int reach_left, int reach_right, float background,
                                           const float *item_weights, float *posterior_out, float *loglik_out,
                                           float *band_counts_out, float *initial_counts_out, void *workspace,
                                           size_t workspace_bytes, int B, int T, int S, int device, void *stream);

/*
 * k-best Viterbi decoding (added within ABI 17): the k best state sequences of every item with their exact scores, on the
 * model torbi_hip_viterbi_decode decodes (torbi_amd/k_best.py, KBEST.md).  Inputs as there: observation (B, T, S) log
 * scores, batch_frames (B,) int32 (clamped to [1, T]), transition (S, S) log [next][prev], initial (S,) log; 1 <= k <= 32.
 * Every state j of frame t keeps a list L_t(j) of (value, back-pointer) entries, all sums in float32:
 *     L_0(j) = [ fl(obs_0[j] + initial[j]) ]
 *     t >= 1: candidates c = fl(L_{t-1}(i)[r] + transition[j][i]) over every prev-state i and rank r of L_{t-1}(i);
 *             L_t(j) = the first min(k, count) in the order (c descending, i ascending, r ascending), each stored as
 *             fl(obs_t[j] + c) with back-pointer (i, r)
 *     result: the first min(k, S^F) entries (L_{F-1}(j)[r], j, r) in the order (value descending, j ascending, r ascending)
 * Rank 0 is torbi_hip_viterbi_decode's path for inputs without NaN or +inf.  indices_out (B, k, T) int32: rank q's path in
 * columns t < F_b, its last state repeated after; scores_out (B, k) fp32: the path's value.  Ranks beyond S^F get score
 * -inf and index -1 in every column.  A NaN or +inf in anything an item reads (initial, the matrix when F_b >= 2, its
 * observation rows t < F_b) gives that item NaN scores and -1 indices.  An item's bits never depend on other items' data.
 *
 * workspace: device scratch (no initialisation, no alignment) of torbi_hip_k_best_workspace_bytes(B, T, S, k) bytes for
 * torbi_hip_k_best (back-pointers: 4 * B * (T - 1) * k * S bytes) and of torbi_hip_k_best_workspace_bytes(B, T, 1, k)
 * bytes for torbi_hip_k_best_uniform.  One launch per frame (general route) or one per call (uniform route), no host
 * synchronisation: with a caller-owned workspace a call can be captured into a graph.
 * The uniform entry point takes a matrix whose every entry is `uniform_value` (torbi_amd passes fl(log(1/S))); it
 * returns the bits of torbi_hip_k_best on that matrix.
 * TORBI_HIP_EINVAL for k outside [1, 32]; TORBI_HIP_ERANGE for S > 16384, B * T > 2^32 or B * T * S > 2^40.
 */
size_t torbi_hip_k_best_workspace_bytes(int B, int T, int S, int k);
int torbi_hip_k_best(const float *observation, const int32_t *batch_frames, const float *transition, const float *initial,
                     int32_t *indices_out, float *scores_out, void *workspace, size_t workspace_bytes, int B, int T, int S,
                     int k, int device, void *stream);
int torbi_hip_k_best_uniform(const float *observation, const int32_t *batch_frames, float uniform_value,
                             const float *initial, int32_t *indices_out, float *scores_out, void *workspace,
                             size_t workspace_bytes, int B, int T, int S, int k, int device, void *stream);

/*
 * The band route of k-best decoding (added within ABI 17): torbi_hip_k_best's indices and scores, bit for bit, for a matrix
 * with transition[j][i] == `background` (bit for bit; -inf or finite) wherever i < j - reach_left or i > j + reach_right, at
 * the cost of the band (csrc/k_best_band.hpp, KBEST.md "Band route").  State j builds its list from its in-band prev-states;
 * where the list is full and its k-th value is strictly greater than the largest out-of-band candidate any state could
 * see, fl(max_i L(i)[0] + background), it is the answer, otherwise the state repeats the scan over all S prev-states.
 * Every frame of a call runs in one launch, G items per workgroup.
 *
 * torbi_hip_k_best_band_covers answers 1 where the route takes a call, else 0, without touching a device: S % 4 == 0,
 * 64 <= S <= 3072, reach_left + reach_right + 4 <= 512 (what torbi_hip_band_reach_over's callers ask about), 1 <= k <= 32,
 * the two list buffers of one item within the LDS -- 8 k (S + reach_left + reach_right) <= 159 * 1024 bytes (k <= 12 at
 * 1440 states and reach 87 / 87) --, and a background that is neither NaN nor +inf.
 * G = min(4, 16 / KMAX) (KMAX: k rounded up to a power of two), halved while 8 G k (S + reach_left + reach_right) exceeds
 * 159 * 1024 and then while ceil(B / G) < 256.
 *
 * torbi_hip_k_best_band_workspace_bytes: torbi_hip_k_best_workspace_bytes's layout with the diagonals,
 * (reach_left + reach_right + 1) * S floats, in place of the transposed matrix, and one verdict word.  No initialisation
 * (flags, counts and the verdict word are set by every call) and no alignment.
 *
 * torbi_hip_k_best_band: arguments as torbi_hip_k_best plus the band.  The promise about the entries outside the band is
 * checked on the device and nothing is read back: where it is broken every item gets NaN scores and -1 indices.
 * EINVAL for a negative reach (and torbi_hip_k_best's cases), EUNSUPPORTED where _covers answers 0.  No host
 * synchronisation and no allocation: a call can be captured into a graph.
 */
int torbi_hip_k_best_band_covers(int B, int T, int S, int k, int reach_left, int reach_right, float background, int device);
size_t torbi_hip_k_best_band_workspace_bytes(int B, int T, int S, int k, int reach_left, int reach_right);
int torbi_hip_k_best_band(const float *observation, const int32_t *batch_frames, const float *transition, const float *initial,
                          int reach_left, int reach_right, float background, int32_t *indices_out, float *scores_out,
                          void *workspace, size_t workspace_bytes, int B, int T, int S, int k, int device, void *stream);

/*
 * Posterior path sampling (added within ABI 17): N whole state sequences per item drawn from P(path | observations) of the
 * model torbi_hip_viterbi_decode decodes, by forward filtering and backward sampling (torbi_amd/sampling.py, SAMPLING.md).
 * Inputs as torbi_hip_forward_backward, and uniforms (B, N, T) fp32: draw n of item b reads uniforms[b][n][t] at frame t, as
 * min(max(u, 0), 1 - 2^-24), NaN as 0.  With a_t the unnormalised filtered rows and E = exp(transition) of that call:
 *     t = F-1:  w[i] = a_{F-1}[i]                 t < F-1:  w[i] = a_t[i] * E[j_{t+1}][i]
 *     Z = sum_i w[i];  j_t = the smallest i with (w[0] + ... + w[i]) > u * Z and w[i] > 0; if there is none (rounding), the
 *     largest i with w[i] > 0
 * The sums run in a fixed tree that depends on S only; a state of weight exactly 0 is never returned.  A draw's bits depend on
 * its item's data and its own T uniforms only.  indices_out (B, N, T) int32: columns t >= F_b repeat j_{F-1}.  loglik_out
 * (B,) fp32: the bits of torbi_hip_forward_backward's L (the same launches).  An item whose L is not finite (-inf: total
 * probability 0; NaN: it reads a NaN or +inf) has -1 in every column of every draw; so has a draw whose Z at some frame is 0
 * or not finite (underflow of the product).
 *
 * workspace: device scratch (no initialisation, no alignment) of torbi_hip_sample_workspace_bytes(B, T, S, N, uniform) bytes:
 * with uniform == 0 the layout of torbi_hip_forward_backward followed by the filter rows (B, T, S) fp32, else (B, T) fp64.  The
 * filter's launches and one sampler launch (uniform: three launches), no allocation and no host synchronisation: a call can
 * be captured into a graph.
 * The uniform entry point takes a matrix whose every entry is `uniform_value`: frames are independent, j_0 ~ softmax(initial
 * + obs_0), j_t ~ softmax(obs_t) under the same rule with w = exp(x - max x), and L as torbi_hip_forward_backward_uniform.
 * TORBI_HIP_EINVAL for a null pointer or N outside [1, 4096]; TORBI_HIP_ERANGE as torbi_hip_forward_backward and for
 * B * N * T > 2^32; TORBI_HIP_EWORKSPACE for a workspace that is too small.  B == 0 returns 0.
 */
size_t torbi_hip_sample_workspace_bytes(int B, int T, int S, int N, int uniform);
int torbi_hip_sample(const float *observation, const int32_t *batch_frames, const float *transition, const float *initial,
                     const float *uniforms, int32_t *indices_out, float *loglik_out, void *workspace, size_t workspace_bytes,
                     int B, int T, int S, int N, int device, void *stream);
int torbi_hip_sample_uniform(const float *observation, const int32_t *batch_frames, float uniform_value, const float *initial,
                             const float *uniforms, int32_t *indices_out, float *loglik_out, void *workspace,
                             size_t workspace_bytes, int B, int T, int S, int N, int device, void *stream);

/*
 * Posterior path sampling on a band (added within ABI 17): torbi_hip_sample for a transition matrix that holds ONE value
 * outside a band, at the cost of the band (SAMPLING.md, "Band route").  The band, `background` and the promise about the
 * entries outside the band are torbi_hip_forward_backward_band's; ebg = exp(background), 0 for -inf.  Frame F-1 draws from
 * the whole row a_{F-1} as torbi_hip_sample does.  Frame t < F-1, with j = j_{t+1}, lo = max(0, j - reach_left) and
 * hi = min(S - 1, j + reach_right), applies the same draw rule to the concatenated weights
 *     [ v[lo] .. v[hi],  ebg * a_t[0] .. ebg * a_t[S-1] ]        v[i] = a_t[i] * max(exp(transition[j][i]) - ebg, 0)
 * and j_t is the state of the chosen slot; Z = sum_i v[i] + ebg * c_t.  loglik_out: the bits of
 * torbi_hip_forward_backward_band's L.  Where the promise is broken every L is NaN and every index -1.
 *
 * torbi_hip_sample_band_covers: 1 where torbi_hip_forward_backward_band_covers answers 1 and 1 <= N <= 4096; it reads no
 * device.  torbi_hip_sample_band_workspace_bytes: torbi_hip_forward_backward_band_workspace_bytes(B, T, S, reach_left,
 * reach_right) plus the filter rows (B, T, S) fp32 on the next 256-byte boundary, whatever N; no initialisation and no
 * alignment of the caller's base.
 * TORBI_HIP_EINVAL for a null pointer, a negative reach or N outside [1, 4096]; TORBI_HIP_ERANGE as torbi_hip_sample;
 * TORBI_HIP_EUNSUPPORTED where _covers answers 0; TORBI_HIP_EWORKSPACE for a workspace that is too small.  B == 0 returns 0.
 * Five launches, no allocation and no host synchronisation: a call can be captured into a graph.
 */
int torbi_hip_sample_band_covers(int B, int T, int S, int N, int reach_left, int reach_right, float background, int device);
size_t torbi_hip_sample_band_workspace_bytes(int B, int T, int S, int N, int reach_left, int reach_right);
int torbi_hip_sample_band(const float *observation, const int32_t *batch_frames, const float *transition, const float *initial,
                          int reach_left, int reach_right, float background, const float *uniforms, int32_t *indices_out,
                          float *loglik_out, void *workspace, size_t workspace_bytes, int B, int T, int S, int N, int device,
                          void *stream);

/*
 * Max-marginals (added within ABI 17): the largest log score of any complete path of item b that is in state j at frame t,
 * on the model torbi_hip_viterbi_decode decodes (torbi_amd/margins.py, MARGINALS.md).  Inputs as there: observation
 * (B, T, S) log scores, batch_frames (B,) int32 (F: clamped to [1, T]), transition (S, S) log [next][prev], initial (S,) log.
 * All sums in float32 with one rounding each:
 *     alpha_0[j] = fl(obs_0[j] + initial[j])
 *     alpha_t[j] = fl(obs_t[j] + max_i fl(alpha_{t-1}[i] + transition[j][i]))                1 <= t < F
 *     beta_{F-1}[i] = +0
 *     beta_t[i]  = max_j fl(transition[j][i] + fl(obs_{t+1}[j] + beta_{t+1}[j]))             0 <= t < F-1
 *     m_t[j]     = fl(alpha_t[j] + beta_t[j])   for t < F,   -inf   for F <= t < T
 *     score      = max_j alpha_{F-1}[j]
 * marginals_out (B, T, S) fp32: m; scores_out (B,) fp32: the score, the bits of rank 0 of torbi_hip_k_best.  A maximum of
 * floats without NaN does not depend on its order, so the values are defined exactly; only the sign of a zero is not
 * (m_{F-1} is stored as alpha_{F-1}).  -inf is an ordinary value: a state no path reaches or leaves has m = -inf, not NaN.
 * A NaN or +inf in anything an item reads (initial, the matrix when F_b >= 2, its observation rows t < F_b) gives that item
 * NaN in every m_t, t < F_b, and a NaN score; its rows t >= F_b stay -inf.  An item's values never depend on other items'
 * data.  Sums of finite inputs that overflow float32 are outside this contract.
 *
 * workspace: device scratch (no initialisation, no alignment) of torbi_hip_max_marginals_workspace_size(B, T, S, uniform)
 * bytes: with uniform == 0 the matrix transposed, two beta rows per item and B + 1 alarm words; else three scalars per item
 * and frame and the alarm words.  It holds no (B, T, S) region: alpha is kept in marginals_out.  The size query answers 256
 * for dimensions below 1 or S > 16384.
 * The general route takes one launch per frame and pass (2 (T - 1) step launches), the uniform route three launches; no
 * allocation and no host synchronisation: a call can be captured into a graph.
 * The uniform entry point takes a matrix whose every entry is `uniform_value` (torbi_amd passes fl(log(1/S))) and returns the
 * values of torbi_hip_max_marginals on that matrix.
 * TORBI_HIP_EINVAL for a null pointer, B < 0, T < 1 or S < 1; TORBI_HIP_ERANGE for S > 16384, B * T > 2^32 or
 * B * T * S > 2^40; TORBI_HIP_EWORKSPACE for a workspace that is too small.  B == 0 returns 0.
 */
size_t torbi_hip_max_marginals_workspace_size(int B, int T, int S, int uniform);
int torbi_hip_max_marginals(const float *observation, const int32_t *batch_frames, const float *transition, const float *initial,
                            float *marginals_out, float *scores_out, void *workspace, size_t workspace_bytes, int B, int T,
                            int S, int device, void *stream);
int torbi_hip_max_marginals_uniform(const float *observation, const int32_t *batch_frames, float uniform_value,
                                    const float *initial, float *marginals_out, float *scores_out, void *workspace,
                                    size_t workspace_bytes, int B, int T, int S, int device, void *stream);

/*
 * Max-marginals on a band (added within ABI 17): the values of torbi_hip_max_marginals, by ==, for a matrix that holds ONE
 * value outside a band, at the cost of the band (MARGINALS.md, "Band route").  The caller states the band --
 * transition[j][i] with j - reach_left <= i <= j + reach_right -- and promises that every entry outside it equals
 * `background` bit for bit.  Rounding is monotone, so the out-of-band candidates of a state are one sum,
 * fl(max over the out-of-band states + background), taken from a prefix and a suffix maximum of the previous row.
 * The promise is checked on the device without waiting for it: where it is broken, every item, whatever its frames, gets NaN
 * in its rows t < F_b and a NaN score.  The non-finite rule is torbi_hip_max_marginals's.
 *
 * torbi_hip_max_marginals_band_covers reads no device and answers 1 for B >= 1, T >= 1, S % 4 == 0, 64 <= S <= 3072,
 * reaches >= 0 with reach_left + reach_right + 4 <= 512, a background that is neither NaN nor +inf, and one item's rows
 * fitting the LDS.
 * workspace: device scratch (no initialisation, no alignment) of torbi_hip_max_marginals_band_workspace_size bytes: the
 * diagonals [reach_left + reach_right + 1][S], B + 1 alarm words and the verdict word; no (B, T, S) region and no beta rows.
 * The size query answers 256 for dimensions below 1, S > 16384, a negative reach or a window above 512.
 * Four launches whatever T (verdict, prepare, every frame of both passes, final); no allocation, no host synchronisation.
 * TORBI_HIP_EINVAL for a null pointer, a negative reach, B < 0, T < 1 or S < 1; TORBI_HIP_ERANGE as torbi_hip_max_marginals;
 * TORBI_HIP_EUNSUPPORTED where _covers answers 0; TORBI_HIP_EWORKSPACE for a workspace that is too small.  B == 0 returns 0.
 * All are answered before a device is touched.
 */
int torbi_hip_max_marginals_band_covers(int B, int T, int S, int reach_left, int reach_right, float background, int device);
size_t torbi_hip_max_marginals_band_workspace_size(int B, int T, int S, int reach_left, int reach_right);
int torbi_hip_max_marginals_band(const float *observation, const int32_t *batch_frames, const float *transition,
                                 const float *initial, int reach_left, int reach_right, float background, float *marginals_out,
                                 float *scores_out, void *workspace, size_t workspace_bytes, int B, int T, int S, int device,
                                 void *stream);

/*
 * Path statistics (added within ABI 17): the exact log score and the transition counts of GIVEN state paths, on the model
 * torbi_hip_viterbi_decode decodes (torbi_amd/paths.py, PATHS.md).  indices (B, K, T) int32: K paths per item; inputs
 * otherwise as torbi_hip_max_marginals (F: batch_frames clamped to [1, T]; transition [next][prev]).  A path q of item b is
 * scored by the decoder's alpha recurrence followed along it, all sums in float32 with one rounding each:
 *     s_0   = fl(obs_0[q_0] + initial[q_0])
 *     s_t   = fl(obs_t[q_t] + fl(s_{t-1} + transition[q_t][q_{t-1}]))                         1 <= t < F
 *     score = s_{F-1}
 * so the score of a path torbi_hip_k_best returns at any rank is that rank's score bit for bit.  The score reads the cells on
 * the path and no others: a NaN, +inf or -inf on the path propagates by plain IEEE arithmetic, one elsewhere in the item
 * does not matter, and there is no item-level non-finite rule.  Columns t >= F are never read.
 * A path that holds an index outside [0, S) at a column t < F is VOID (the -1 ranks of torbi_hip_k_best, the -1 rows of
 * torbi_hip_sample): its score is -inf and it adds nothing to any count.
 * Counts, with path_weights w (B, K) fp32 (NULL: all ones), in the orientation of torbi_hip_forward_backward_counts:
 *     transition_counts_out[j][i] = sum over b, k of w[b][k] * #{1 <= t < F : q_t = j, q_{t-1} = i}          (S, S) fp32
 *     initial_counts_out[j]       = sum over b, k of w[b][k] * [q_0 = j]                                     (S,)   fp32
 * accumulated in float64 (the weights converted exactly, hardware float64 atomics) and rounded to float32 once: unweighted
 * counts, and counts under weights that are small multiples of a power of two, are exact whatever the order of the adds;
 * with general non-negative weights the result is within one float32 ulp of the exact sum.
 *
 * transition == NULL: the matrix whose every entry is `uniform_value` (torbi_amd passes fl(log(1/S))).
 * scores_out == NULL: counts only; then observation, transition and initial may be NULL (nothing of the model is read).
 * transition_counts_out == NULL and initial_counts_out == NULL (both): scores only; then the workspace size is 0 and a NULL
 * workspace is accepted.
 * workspace: device scratch (no initialisation, no alignment) of torbi_hip_path_statistics_workspace_size(B, T, S, K,
 * counts) bytes: the S * S + S float64 accumulators, which the call zeroes itself on the stream; 0 with counts == 0, 256
 * for dimensions below 1 or S > 16384.
 * One launch for every path (one wavefront per path), plus with counts one memset before and one rounding launch behind it;
 * no allocation and no host synchronisation: a call can be captured into a graph, and the graph is linear.
 * TORBI_HIP_EINVAL for any other null pointer (one count output without the other, no output at all, a missing workspace
 * with counts), B < 0, T < 1, S < 1 or K < 1; TORBI_HIP_ERANGE for S > 16384, B * K > 2^31 - 4, B * K * T > 2^40 or
 * B * T * S > 2^40; TORBI_HIP_EWORKSPACE for a workspace that is too small.  All are answered before anything is launched.
 * B == 0 launches nothing and returns 0.
 */
size_t torbi_hip_path_statistics_workspace_size(int B, int T, int S, int K, int counts);
int torbi_hip_path_statistics(const float *observation, const int32_t *batch_frames, const float *transition, float uniform_value,
                              const float *initial, const int32_t *indices, const float *path_weights, float *scores_out,
                              float *transition_counts_out, float *initial_counts_out, void *workspace, size_t workspace_bytes,
                              int B, int T, int S, int K, int device, void *stream);

/*
 * Path entropy (added within ABI 17): the entropy, in nats, of the posterior over whole state paths of every item,
 *     H_b = - sum over every path q of item b of P(q | o_b) log P(q | o_b),
 * on the model torbi_hip_forward_backward takes (torbi_amd/entropy.py, ENTROPY.md): observation (B, T, S) log scores,
 * batch_frames (B,) int32 (F: clamped to [1, T]), transition (S, S) log [next][prev] (-inf a zero probability; it need not
 * be stochastic), initial (S,) log.  The forward-only recursion of Hernando, Crespi and Cybenko on the scaled forward pass,
 * with E = exp(transition), G = E o transition (0 where transition = -inf), p_t the filtered distribution, xlogx(0) = 0:
 *     h_0 = 0,   u_t[j] = p_t[j] h_t[j] - xlogx(p_t[j]),   d = E p_{t-1}
 *     h_t[j] = log d[j] + ((E u_{t-1})[j] - (G p_{t-1})[j]) / d[j]        (0 where d[j] = 0)
 *     prefix_t = sum_j u_t[j]   (the entropy of q_0 .. q_t given o_0 .. o_t),   H = prefix_{F-1}
 * entropy_out (B,) fp32: H.  prefix_out (B, T) fp32 or null: prefix_t, 0 for t >= F_b.  loglik_out (B,) fp32: the
 * log-likelihood of torbi_hip_forward_backward.  Products in float32 on the matrix pipe; the sums over states that give
 * prefix_t and the sum over frames that gives the log-likelihood in float64, rounded once.  The entropy is what the
 * arithmetic gives: it is not clamped at 0.  A NaN or +inf in anything an item reads (initial, the matrix when F_b >= 2, its
 * observation rows t < F_b) gives that item a NaN log-likelihood, a NaN entropy and NaN prefix entries t < F_b; an item of
 * total probability 0 has log-likelihood -inf and the same NaNs.  An item's bits never depend on other items' data, on the
 * batch size or on what the workspace held.
 *
 * workspace: device scratch (no initialisation, no alignment) of torbi_hip_path_entropy_workspace_size(B, T, S, uniform)
 * bytes: with uniform == 0 two padded copies of the matrix, four scalars per item and frame, and four rows and two rows of
 * 32-row partial sums per item; else two float64 per item and frame.  It holds no (B, T, S) region.  The size query answers
 * 256 for dimensions below 1 or S > 16384.
 * The general route takes two launches per frame, the uniform route two launches; no allocation and no host synchronisation:
 * a call can be captured into a graph.
 * The uniform entry point takes a matrix whose every entry is `uniform_value` (torbi_amd passes fl(log(1/S))): frames are
 * independent there, prefix_t is the running sum of the entropies of softmax(obs_s) (s = 0: softmax(initial + obs_0)).
 * TORBI_HIP_EINVAL for a null pointer other than prefix_out, B < 0, T < 1 or S < 1; TORBI_HIP_ERANGE for S > 16384,
 * B * T > 2^32, B * T * S > 2^40 or B > 32 * 65535; TORBI_HIP_EWORKSPACE for a workspace that is too small.  All are
 * answered before a device is touched.  B == 0 launches nothing and returns 0.
 */
size_t torbi_hip_path_entropy_workspace_size(int B, int T, int S, int uniform);
int torbi_hip_path_entropy(const float *observation, const int32_t *batch_frames, const float *transition, const float *initial,
                           float *entropy_out, float *prefix_out, float *loglik_out, void *workspace, size_t workspace_bytes,
                           int B, int T, int S, int device, void *stream);
int torbi_hip_path_entropy_uniform(const float *observation, const int32_t *batch_frames, float uniform_value,
                                   const float *initial, float *entropy_out, float *prefix_out, float *loglik_out,
                                   void *workspace, size_t workspace_bytes, int B, int T, int S, int device, void *stream);

/*
 * Path entropy on a band with one value outside it (added within ABI 17; torbi_amd/entropy.py forward_entropy_banded,
 * ENTROPY.md "Band route"): what torbi_hip_path_entropy computes, for a matrix of which the caller states a band
 *     transition[j][i] ([next][prev]) with j - reach_left <= i <= j + reach_right
 * and promises that every entry outside it equals `background` bit for bit, as for torbi_hip_forward_backward_band.  With
 * ebg = exp(background) and gbg = ebg * background (both 0 for -inf) every product of the recursion splits into the band
 * and one constant,
 *     (E x)[j] = sum_{i in band(j)} (E[j][i] - ebg) x[i] + ebg * sum_i x[i],   (G x)[j] likewise with G - gbg and gbg,
 * so a frame costs 3 W multiplies per state, W = reach_left + reach_right + 1 (reaches clamped to S - 1).  The division by
 * the row sum is deferred: the kernel carries a_t (sum c_t) and v_t = a_t h_t - xlogx(a_t), from which
 * prefix_t = (sum_j v_t[j]) / c_t + log c_t in float64.  The outputs, the non-finite rules and the independence of an
 * item's bits from the batch are torbi_hip_path_entropy's; the values agree with it within the bound of ENTROPY.md, not bit
 * for bit, and a single-path model gives 0 within that bound, not exactly.  The promise is checked on the device without the
 * host waiting for it: where it is broken every item has a NaN log-likelihood, a NaN entropy and NaN prefix entries t < F_b.
 *
 * torbi_hip_path_entropy_band_covers reads no device and answers 1 for 1 <= S <= 4096, min(W, S) <= 64, a background that is
 * neither NaN nor +inf, B >= 1, T >= 1 within torbi_hip_path_entropy's limits, and one item's rows within the kernel's LDS.
 * workspace: device scratch (no initialisation, no alignment) of torbi_hip_path_entropy_band_workspace_size bytes: the two
 * sets of diagonals [W][S up to 64], three scalars per item and frame (row maxima, row sums, the prefix where prefix_out is
 * null) and the promise flag.  It holds no (B, T, S) region.  The size query answers 256 for dimensions below 1, a negative
 * reach or S > 4096.
 * Four launches whatever T, no allocation and no host synchronisation: a call can be captured into a graph.
 * TORBI_HIP_EINVAL for a null pointer other than prefix_out, a negative reach, B < 0, T < 1 or S < 1; TORBI_HIP_ERANGE for a
 * shape beyond torbi_hip_path_entropy's limits; TORBI_HIP_EUNSUPPORTED where _covers answers 0; TORBI_HIP_EWORKSPACE for a
 * workspace that is too small; in that order and all before a device is touched.  B == 0 launches nothing and returns 0.
 */
int torbi_hip_path_entropy_band_covers(int B, int T, int S, int reach_left, int reach_right, float background, int device);
size_t torbi_hip_path_entropy_band_workspace_size(int B, int T, int S, int reach_left, int reach_right);
int torbi_hip_path_entropy_band(const float *observation, const int32_t *batch_frames, const float *transition,
                                const float *initial, int reach_left, int reach_right, float background, float *entropy_out,
                                float *prefix_out, float *loglik_out, void *workspace, size_t workspace_bytes, int B, int T, int S,
                                int device, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TORBI_HIP_H */
