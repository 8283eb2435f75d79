/*
 * torchain_hip.h -- C ABI of the MI355X-native LF-MMI chain loss (libtorchain_hip.so).
 *
 * This is the drop-in boundary for ONE path of nttcslab-sp/torchain: the chain objective and its
 * derivative.  Every entry point names the reference interface it replaces (paths relative to the
 * reference repository).  Plain pointers and sizes only: no torch / TH types, no C++ exceptions
 * across the boundary; all functions that can fail return 0 (TC_OK) or a negative TC_ERR_* code.
 *
 * Conventions (same as the reference, torchain/functions.py:27-30, src/my_lib_chain.cpp:104-136):
 *   nnet_output is a (num_sequences*frames_per_sequence) x num_pdfs fp32 matrix in DEVICE memory,
 *   row = frame * num_sequences + sequence ("all sequences for frame 0; all for frame 1; ..."),
 *   unit column stride, row stride >= num_pdfs (in elements).  All tensors are borrowed for the
 *   duration of the call and never retained.  Work is enqueued on `stream` (a hipStream_t passed as
 *   void*) of `device`; no entry point synchronises the host.
 */
#ifndef TORCHAIN_HIP_H_
#define TORCHAIN_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TC_OK 0
#define TC_ERR_INVALID_ARGUMENT (-1)  /* null pointer, bad dims/stride, leaky not in (0,1)        */
#define TC_ERR_BAD_FST (-2)           /* state/label out of range, arcs not state-major, ...      */
#define TC_ERR_UNSUPPORTED (-3)       /* graph or supervision too large for the on-chip layout    */
#define TC_ERR_WORKSPACE (-4)         /* workspace missing or smaller than tc_*_workspace_bytes   */
#define TC_ERR_HIP (-5)               /* a HIP runtime call failed (see tc_last_hip_error)        */
#define TC_ERR_IO (-6)                /* file could not be read / is not an OpenFst vector FST    */
#define TC_ERR_NOT_SEPARABLE (-7)     /* merged supervision FST does not factor per sequence      */

typedef struct tc_den_graph tc_den_graph;     /* replaces the void* to kaldi::chain::DenominatorGraph */
typedef struct tc_supervision tc_supervision; /* replaces the void* to kaldi::chain::Supervision      */

/* Replaces my_lib_test_chain (src/my_lib.h:45, src/my_lib_chain.cpp:138-213), the reference's native self test: runs
 * the full objective on a small synthetic problem on `device` and checks the properties its Kaldi tests assert
 * (src/chain-supervision-test.hpp:239-341, 388-463).  Returns TC_OK, a negative TC_ERR_* if the library could not
 * run, or the number of the property that failed: 1 weight = w * S * T; 2 objf <= 0 for a numerator inside the
 * denominator; 3 derivative rows sum to ~0; 4 finite differences agree with the derivative; 5 the objective is the
 * failure value -10 * weight.  report6 (nullable, host): objf, weight, worst |row sum|, predicted and observed change
 * of objf under the test perturbation, l2_term.  A C-only integrator can validate an install with this one call. */
int tc_self_test(int device, void *stream, float *report6);

const char *tc_strerror(int code);
int tc_version(void);
int tc_last_hip_error(void);

/* ---- denominator graph ------------------------------------------------------------------- */

/* Replaces my_lib_denominator_graph_new (src/my_lib.h:29, src/my_lib_example.cpp:129-134) for an FST
 * already in memory.  Arcs are listed state-major in the order an OpenFst ArcIterator yields them;
 * ilabel = pdf_id + 1; weights are tropical (-log prob); final_weight[s] = +inf for a non-final
 * state.  Builds the transition tables, the 100-iteration initial-probability estimate and the
 * wavefront schedules used by the kernels.  Host only; touches no GPU. */
int tc_den_graph_create(tc_den_graph **out, int32_t num_states, int64_t num_arcs, const int32_t *arc_src,
                        const int32_t *arc_dst, const int32_t *arc_ilabel, const float *arc_weight,
                        const float *final_weight, int32_t start_state, int32_t num_pdfs);

/* Replaces my_lib_denominator_graph_new(rxfilename, num_pdf) (src/my_lib.h:29) for a den.fst on disk:
 * reads an OpenFst binary VectorFst<StdArc> (what fst::ReadFstKaldi accepts) from a plain filename or
 * from a Kaldi-style piped rxfilename ("gunzip -c den.fst.gz |") and calls tc_den_graph_create. */
int tc_den_graph_read(tc_den_graph **out, const char *rxfilename, int32_t num_pdfs);

/* Replaces my_lib_denominator_graph_free (src/my_lib.h:30). */
void tc_den_graph_free(tc_den_graph *graph);

int32_t tc_den_graph_num_states(const tc_den_graph *graph);
int64_t tc_den_graph_num_arcs(const tc_den_graph *graph);
int32_t tc_den_graph_num_pdfs(const tc_den_graph *graph);
/* Copies the num_states initial probabilities ([K] DenominatorGraph::InitialProbs) to host memory. */
int tc_den_graph_initial_probs(const tc_den_graph *graph, float *out_host);

/* Uploads the graph's immutable tables to `device` (idempotent, thread-safe).  The hot calls do this
 * on first use; call it at init to keep allocation out of the first step.  One copy per device:
 * this is what makes a single graph handle usable from every rank/GPU (the reference cannot:
 * example/chime5/parallel_train.py:27-31,47). */
int tc_den_graph_prepare(tc_den_graph *graph, int device);

/* ---- supervision -------------------------------------------------------------------------- */

/* Replaces my_lib_supervision_new (src/my_lib.h:21, src/my_lib_example.cpp:71-76): builds the handle
 * from the five fields of [K] chain::Supervision the path uses (weight, num_sequences,
 * frames_per_sequence, label_dim, fst).  The FST is the merged, epsilon-free, time-sorted acceptor
 * in CSR form: state i owns arcs [arc_begin[i], arc_begin[i+1]); start state 0; ilabel = pdf_id + 1;
 * final_weight[i] = +inf when state i is not final.  The handle splits the FST into its
 * num_sequences independent per-sequence acceptors (TC_ERR_NOT_SEPARABLE if it does not factor).
 * Size: a sequence may have any number of states.  The numerator keeps a sequence in LDS when it fits (16 * states +
 * 4 * arcs + 4 * unique (frame, pdf) <= 160 KB, about 6000 states) and otherwise a window of two time levels, with a
 * log-alpha history of 8 bytes per state in the supervision's device slot; the functions that run the numerator return
 * TC_ERR_UNSUPPORTED only when a single time level does not fit (32 * states + 4 * arcs + 4 * unique of the level, about
 * 4000 states) or the history exceeds 4 GiB.  tc_supervision_stats tells which, on the host. */
int tc_supervision_create(tc_supervision **out, float weight, int32_t num_sequences,
                          int32_t frames_per_sequence, int32_t label_dim, int32_t num_states,
                          const int32_t *arc_begin, const int32_t *arc_ilabel, const float *arc_weight,
                          const int32_t *arc_nextstate, const float *final_weight);

/* End-to-end ("flat-start") supervision: [K] Supervision::e2e_fsts, one epsilon-free acceptor per sequence, not
 * unfolded in time (self-loops and cycles allowed; every arc consumes one frame).  The per-sequence CSRs are
 * concatenated: sequence s owns states [seq_state_begin[s], seq_state_begin[s+1]) (seq_state_begin[0] = 0), its
 * local state i owns arcs [arc_begin[g], arc_begin[g+1]) of g = seq_state_begin[s] + i, arc_begin has
 * seq_state_begin[S] + 1 entries starting at 0; start[s] and arc_nextstate are local to the sequence;
 * ilabel = pdf_id + 1; arc_weight / final_weight are tropical costs (+inf final: not final).  The numerator is
 * [K] GenericNumeratorComputation (num_e2e_kernels.hip); the denominator, the workspace sizes and every entry point
 * taking a supervision are those of the regular one.  TC_ERR_BAD_FST: label 0 or > label_dim, next state or start out
 * of range, NaN or -inf cost, a sequence without a final state;  TC_ERR_UNSUPPORTED: a sequence beyond
 * TC_E2E_MAX_STATES states, TC_E2E_MAX_ARCS arcs or TC_E2E_MAX_PDFS distinct pdfs,
 * num_sequences * frames_per_sequence above 2^26, or a kernel scratch -- (T + 1) x total states x 8 bytes of alpha
 * history + T x total distinct pdfs (summed over sequences) x 4 bytes, held with the supervision's device tables --
 * above 4 GiB. */
#define TC_E2E_MAX_STATES 2048
#define TC_E2E_MAX_ARCS 8192
#define TC_E2E_MAX_PDFS 1024
int tc_supervision_create_e2e(tc_supervision **out, float weight, int32_t num_sequences, int32_t frames_per_sequence,
                              int32_t label_dim, const int32_t *seq_state_begin, const int32_t *start,
                              const int32_t *arc_begin, const int32_t *arc_ilabel, const float *arc_weight,
                              const int32_t *arc_nextstate, const float *final_weight);
/* 1 for a handle of tc_supervision_create_e2e or tc_supervision_create_e2e_ragged, else 0. */
int32_t tc_supervision_is_e2e(const tc_supervision *supervision);

/* End-to-end minibatch of UNEQUAL sequence lengths ("ragged"): tc_supervision_create_e2e with one frame count per
 * sequence, frames_per_sequence[s] >= 1 (host memory, num_sequences entries; a smaller entry: TC_ERR_INVALID_ARGUMENT).
 * T = the longest length is the handle's tc_supervision_num_frame and the T of every tensor shape, row count
 * (num_rows = num_sequences * T, row t * num_sequences + s), workspace size and of the size limits above; frames
 * t >= frames_per_sequence[s] of sequence s are PADDING.  Every entry that takes a supervision takes such a handle:
 *   - nothing in the padding of an input influences any output (NaN and inf included);
 *   - every padding element of an output (deriv, xent_deriv, grad, xent_grad, in every layout and dtype, with
 *     deriv_weights, with the out-of-range penalty, on the soft-failure route) is +0.0;
 *   - the objective's weight is weight * sum of the lengths, its failure value -10 times that, the l2 term sums over the
 *     sequences' own frames; a sequence with no path of exactly its own number of arcs fails the minibatch softly.
 * The lengths travel to the device with the tables (no allocation, no synchronisation once the pool is warm; the step
 * stays capturable).  On a tied graph a batch of 8 sequences up to half the device's CUs runs on two workgroups per
 * sequence that meet at half the sequence's own length when a derivative is asked for (the workspace is the same;
 * "no_mitm" or "no_phase_split" set: not; tc_debug_counter("ragged_two_cu_launches")); every other batch takes the
 * one-workgroup-per-sequence kernel of the graph's class -- the two-pass form and the two-sequence kernel are never
 * taken, and below 8 sequences no launch switch decides anything -- and a graph on the streamed
 * path (tc_den_graph_stats) is refused: TC_ERR_UNSUPPORTED from every entry, before anything is launched.  A handle made
 * here is ragged also when all its lengths are equal; tc_supervision_create_e2e's handles are untouched.
 * tc_supervision_frames: the num_sequences lengths (all equal to tc_supervision_num_frame for any other handle) into host
 * memory.  tc_supervision_is_ragged: 1 for a handle of tc_supervision_create_e2e_ragged or tc_supervision_create_ragged,
 * else 0.
 * tc_debug_counter("ragged_steps") counts the objective calls made on a ragged handle.
 * Regular supervisions of unequal lengths: tc_supervision_create_ragged below. */
int tc_supervision_create_e2e_ragged(tc_supervision **out, float weight, int32_t num_sequences,
                                     const int32_t *frames_per_sequence, int32_t label_dim,
                                     const int32_t *seq_state_begin, const int32_t *start, const int32_t *arc_begin,
                                     const int32_t *arc_ilabel, const float *arc_weight, const int32_t *arc_nextstate,
                                     const float *final_weight);
int tc_supervision_frames(const tc_supervision *supervision, int32_t *frames_host);
int32_t tc_supervision_is_ragged(const tc_supervision *supervision);

/* End-to-end supervisions of ANY size the device can walk: tc_supervision_create_e2e (seq_frames == NULL: every sequence
 * has frames_per_sequence frames) and tc_supervision_create_e2e_ragged (seq_frames: one length >= 1 per sequence, host
 * memory; frames_per_sequence is not read) in one entry, with the same input, the same validation in the same order
 * (TC_ERR_BAD_FST before any size rule) and the same tables, but without TC_E2E_MAX_STATES / _ARCS / _PDFS.  A sequence is
 * refused on size (TC_ERR_UNSUPPORTED) only when
 *     16 * ceil4(states) + 4 * ceil4(distinct pdfs) + 2048 > 163840        (ceil4: rounded up to a multiple of 4)
 * -- two double score vectors and the frame's y per distinct pdf in LDS: 8192 states with 7680 distinct pdfs, 10108 states
 * with 4 -- and its arc count is not limited beyond the tables' int32 offsets.  The rule is per sequence: the kernels lay
 * their LDS out with each sequence's own sizes, so a batch's largest state count and its largest pdf count may belong to
 * two sequences (10108 states / 4 pdfs beside 8192 / 7680 is taken, by the numerator and by tc_supervision_best_path).  The rules on num_sequences * frames and on
 * the 4 GiB of kernel scratch stand as above.
 * A handle whose sequences all fit the three limits is the handle the two entries above make: same kernel
 * (num_e2e_kernels.hip), same launches, same pool slot, same bits.  One with a sequence beyond them takes
 * num_e2e_large_kernels.hip -- the same arithmetic in the same orders, the arc occupations in the supervision's pool slot
 * (4 bytes per arc more) instead of LDS -- in every entry that takes a supervision: the objective and its derivative
 * beside the denominator or in line, the cross-entropy outputs, 16-bit (B, C, T) inputs, ragged lengths, the per-sequence
 * step, tc_supervision_best_path.  tc_debug_counter("num_e2e_large_launches") counts its launches.
 * The two older entries keep their refusal; tc_rand_reader_* and the egs readers build their handles through them. */
int tc_supervision_create_e2e_any(tc_supervision **out, float weight, int32_t num_sequences, int32_t frames_per_sequence,
                                  const int32_t *seq_frames, int32_t label_dim, const int32_t *seq_state_begin,
                                  const int32_t *start, const int32_t *arc_begin, const int32_t *arc_ilabel,
                                  const float *arc_weight, const int32_t *arc_nextstate, const float *final_weight);
/* What the numerator will do with an end-to-end supervision, known on the host (tc_supervision_stats' counterpart; a regular
 * handle: TC_ERR_INVALID_ARGUMENT).  out8: sequences; the most states, arcs and distinct pdfs of one sequence; the LDS bytes
 * the resident kernel would need for them and the LDS bytes the large kernel needs (the most of one sequence); the bytes of kernel scratch in the
 * handle's pool slot (history, y / posteriors and, on the large route, the arc occupations, each rounded up to 256); the
 * route: 0 resident, 1 large ("force_num_e2e_large" as it stands at this call). */
int tc_supervision_e2e_stats(const tc_supervision *supervision, int64_t *out8);

/* Regular (time-unfolded) supervisions of UNEQUAL sequence lengths: one epsilon-free acceptor per sequence, the acceptors
 * concatenated the way tc_supervision_create_e2e_ragged takes its input (sequence s owns states [seq_state_begin[s],
 * seq_state_begin[s+1]); arc_begin has seq_state_begin[S] + 1 entries starting at 0, positions in the concatenated arc
 * arrays; arc_nextstate is local to the sequence; ilabel = pdf_id + 1; tropical costs, final_weight = +inf: not final).
 * Each sequence is what tc_supervision_create accepts with num_sequences = 1 and frames_per_sequence[s] frames: state 0 its
 * start, states numbered in time order, every path exactly frames_per_sequence[s] arcs long, final costs on the last level
 * only.  Nothing is merged, split or re-weighted: a sequence's tables are those tc_supervision_create builds for it alone,
 * and the numerator gives, for every sequence of the batch, the bits it gives on that sequence alone.
 * The handle is a ragged one in every respect stated above for tc_supervision_create_e2e_ragged -- T = the longest length,
 * padding, +0, the objective's weight, the denominator's forms, the refusal of graphs on the streamed path -- also when all
 * its lengths are equal, and tc_supervision_is_e2e is 0.  tc_supervision_stats works on it: "frames" is the longest length,
 * the sizes are the batch's maxima, and they choose between the resident and the level-windowed kernel as for
 * tc_supervision_create.
 * TC_ERR_INVALID_ARGUMENT: a length below 1.  TC_ERR_BAD_FST: a sequence whose paths are not all exactly its own number
 * of arcs long, a label outside 1 .. label_dim, a next state out of range, states out of time order.  TC_ERR_UNSUPPORTED:
 * num_sequences * the longest length above 2^26, or a log-alpha history (8 bytes per state of the batch) above 4 GiB. */
int tc_supervision_create_ragged(tc_supervision **out, float weight, int32_t num_sequences,
                                 const int32_t *frames_per_sequence, int32_t label_dim,
                                 const int32_t *seq_state_begin, const int32_t *arc_begin, const int32_t *arc_ilabel,
                                 const float *arc_weight, const int32_t *arc_nextstate, const float *final_weight);

/* Merges the supervision FSTs of a minibatch's examples into the one acceptor tc_supervision_create takes: what the
 * reference reaches natively through kaldi::nnet3::MergeChainExamples -> [K] chain::AppendSupervision
 * (src/my_lib_example_rand.cpp:160).  Host memory only, no GPU needed.  The pieces arrive concatenated: piece k has
 * piece_num_states[k] states and spans piece_num_frames[k] = num_sequences * frames_per_sequence frames; its CSR
 * offsets (num_states + 1 entries, starting at 0) follow those of the pieces before it in `arc_begin`, its arcs and
 * final weights likewise (nextstate local to the piece; +inf = not final).  fst::Concat + RmEpsilon + breadth-first
 * renumbering: a final state f of piece k-1 receives copies of piece k's start arcs with weight w_f + arc weight and
 * stops being final, piece k's start state disappears, states are numbered in time order.  The caller provides the
 * output arrays (cap_states + 1 / cap_arcs entries; TC_ERR_WORKSPACE if too small: sum of the pieces' states, and
 * sum of the arcs + for every boundary (final states before it) x (start arcs behind it), always suffice).
 * TC_ERR_BAD_FST: a piece is not a connected acceptor whose paths all have piece_num_frames[k] arcs. */
int tc_supervision_append(int32_t num_pieces, const int32_t *piece_num_states, const int32_t *piece_num_frames,
                          const int32_t *arc_begin, const int32_t *arc_ilabel, const float *arc_weight,
                          const int32_t *arc_nextstate, const float *final_weight, int64_t cap_states,
                          int64_t cap_arcs, int32_t *out_num_states, int64_t *out_num_arcs, int32_t *out_arc_begin,
                          int32_t *out_ilabel, float *out_weight, int32_t *out_nextstate, float *out_final);

/* ---- chain examples ("egs") on the host: reading and merging a minibatch -------------------------------------- */

/* Replaces the reading half of the reference's random-access minibatch reader (src/my_lib_example_rand.cpp:35-177:
 * RandomAccessNnetChainExampleReader::Value per key + kaldi::nnet3::MergeChainExamples): opens the n scp entries
 * (paths[i], byte offsets[i] of the "\0B" binary marker; offsets NULL or < 0 = start of file), parses the binary
 * <Nnet3ChainEg> objects (NnetIo with FM/DM/CM/CM2/CM3 matrices, NnetChainSupervision with a compact_acceptor FST,
 * <DW>/<DW2> deriv weights) and, for n > 1 or merge_single != 0, merges them: every input stacked example by example
 * with n = the example's position, supervisions appended as by tc_supervision_append, output indexes and
 * deriv_weights frame-major.  Host memory only, no GPU, thread-safe; TC_ERR_IO (file), TC_ERR_BAD_FST (format; text in
 * tc_example_last_error, per thread), TC_ERR_INVALID_ARGUMENT (examples that cannot be merged). */
typedef struct tc_example tc_example;
int tc_example_read(const char *const *paths, const int64_t *offsets, int32_t n, int merge_single, tc_example **out);
void tc_example_free(tc_example *example);
const char *tc_example_last_error(void);
/* Sequential archives, what the reference reads through SequentialNnetChainExampleReader (src/my_lib_example.cpp:35-69):
 * rxfilename is a path or "command |" (popen).  tc_archive_next returns 1 and one example as stored (not merged; its key,
 * NUL-terminated, in key[0..key_cap)), 0 at the end of the archive, or a negative TC_ERR_* (text in
 * tc_example_last_error).  tc_archive_close returns TC_ERR_IO when a piped command exited with an error. */
typedef struct tc_archive tc_archive;
int tc_archive_open(const char *rxfilename, tc_archive **out);
int tc_archive_next(tc_archive *archive, char *key, int32_t key_cap, tc_example **out);
int tc_archive_close(tc_archive *archive);
/* out2 = {number of inputs, number of outputs}. */
int tc_example_counts(const tc_example *example, int32_t *out2);
/* Input j (reference my_lib_example_feats, src/my_lib_example.cpp:79-100): pointers into the object, valid until
 * tc_example_free; indexes = num_indexes x (n, t, x); features = rows x cols, row-major.  Any out pointer may be NULL. */
int tc_example_input(const tc_example *example, int32_t j, const char **name, int32_t *rows, int32_t *cols,
                     int32_t *num_indexes, const float **features, const int32_t **indexes);
/* Output j (reference my_lib_supervision_new / my_lib_example_reader_indexes, src/my_lib_example.cpp:71-76, 102-127):
 * dims5 = {num_sequences, frames_per_sequence, label_dim, num_states, num_arcs}; the FST arrays are what
 * tc_supervision_create takes. */
int tc_example_output(const tc_example *example, int32_t j, const char **name, int32_t *num_indexes,
                      const int32_t **indexes, const float **deriv_weights, float *weight, int32_t *dims5,
                      const int32_t **arc_begin, const int32_t **ilabel, const float **arc_weight,
                      const int32_t **nextstate, const float **final_weight);
/* Output j's kind: *is_e2e = 1 for an end-to-end supervision ([K] Supervision::e2e_fsts, `<End2End>` true in the egs).
 * Then tc_example_output's arrays hold the per-sequence FSTs concatenated (dims5[3] = their total states, dims5[4] =
 * their total arcs) and seq_state_begin (num_sequences + 1) / start (num_sequences) complete what
 * tc_supervision_create_e2e takes; both are NULL for a regular output.  A minibatch that mixes e2e and regular
 * examples does not merge (tc_example_read: TC_ERR_INVALID_ARGUMENT). */
int tc_example_output_e2e(const tc_example *example, int32_t j, int32_t *is_e2e, const int32_t **seq_state_begin,
                          const int32_t **start);

/* Random-access minibatch reader: my_lib_example_rand_reader_new / _reset / _num_batch / _num_data / _next / _free,
 * my_lib_example_rand_feats and my_lib_supervision_rand_new of the reference (src/my_lib.h:8-17 over RandReader,
 * src/my_lib_example_rand.cpp:35-177).  `scp_path` holds "key path:offset" lines; `len_file` ("" or NULL: scp_path +
 * ".len"; absent: the lengths are read from the examples) holds "key frames_per_sequence" pairs.  Examples of equal
 * length are grouped into minibatches of `batchsize` (the last of a length may be smaller), shuffled inside and across
 * the lengths by a std::mt19937 seeded with `seed`.  tc_rand_reader_new_ordered's `order`:
 *   TC_RAND_ORDER_SORTED (tc_rand_reader_new): lengths ascending, Fisher-Yates with the draw (engine() * n) >> 32 -- the same on
 *                  every platform;
 *   TC_RAND_ORDER_REFERENCE: the reference's statement on its own library calls (src/my_lib_example_rand.cpp:119-141):
 *                  lengths in the iteration order of a std::unordered_map<size_t, ...> filled in file order, every
 *                  length's keys copied out and passed to std::shuffle, the batches passed to std::shuffle -- the batch
 *                  lists of the reference built against the same standard library (libstdc++), seed for seed and epoch
 *                  for epoch; rank / world sharding applies on top.
 * New here:
 *   rank / world : every rank forms the same shuffled list and takes batches rank, rank + world, ...; all ranks get
 *                  floor(batches / world) of them per epoch (reference antecedent: example/chime5/parallel_train.py:26-75)
 *   lookahead    : that many worker threads read, parse, merge ([K] MergeChainExamples) and build the supervision
 *                  handles of the next batches while the caller uses the current one (0: everything inside _next)
 * tc_rand_reader_next: 1 = moved to the next minibatch, 0 = the epoch is over, negative TC_ERR_* (text in
 * tc_rand_reader_last_error).  The reader starts BEFORE its first minibatch.  tc_rand_reader_example: the current merged
 * minibatch (tc_example_input / _output; owned by the reader, valid until the next _next / _reset / _free);
 * tc_rand_reader_supervision_new: a supervision handle of it that the caller frees (tc_supervision_free);
 * tc_rand_reader_take_example: the current minibatch itself, the caller's to free (tc_example_free) -- for callers
 * that keep its arrays beyond the next _next.
 * tc_rand_reader_batch_keys: the keys of this rank's batch `batch` of the current epoch, space-separated, into buf;
 * returns their number.  Host only. */
typedef struct tc_rand_reader tc_rand_reader;
#define TC_RAND_ORDER_SORTED 0
#define TC_RAND_ORDER_REFERENCE 1
int tc_rand_reader_new(const char *scp_path, int seed, int batchsize, const char *len_file, int rank, int world,
                       int lookahead, tc_rand_reader **out);
int tc_rand_reader_new_ordered(const char *scp_path, int seed, int batchsize, const char *len_file, int rank, int world,
                               int lookahead, int order, tc_rand_reader **out);
/* device >= 0: the look-ahead threads also stage every supervision they build for that GPU (tc_supervision_stage). */
int tc_rand_reader_set_device(tc_rand_reader *reader, int device);
int tc_rand_reader_reset(tc_rand_reader *reader);
int tc_rand_reader_num_batch(const tc_rand_reader *reader);
int tc_rand_reader_num_data(const tc_rand_reader *reader);
int tc_rand_reader_next(tc_rand_reader *reader);
int tc_rand_reader_example(const tc_rand_reader *reader, const tc_example **out);
int tc_rand_reader_supervision_new(tc_rand_reader *reader, tc_supervision **out);
int tc_rand_reader_take_example(tc_rand_reader *reader, tc_example **out);
int tc_rand_reader_batch_keys(const tc_rand_reader *reader, int32_t batch, char *buf, int32_t cap);
void tc_rand_reader_free(tc_rand_reader *reader);
const char *tc_rand_reader_last_error(void);

/* Replaces my_lib_supervision_free (src/my_lib.h:22). */
void tc_supervision_free(tc_supervision *supervision);
/* Replace my_lib_supervision_num_pdf / _num_sequence / _num_frame (src/my_lib.h:23-25). */
int32_t tc_supervision_num_pdf(const tc_supervision *supervision);
int32_t tc_supervision_num_sequence(const tc_supervision *supervision);
int32_t tc_supervision_num_frame(const tc_supervision *supervision);
float tc_supervision_weight(const tc_supervision *supervision);
/* What the numerator will do with a regular supervision, host only (nothing touches a GPU): out[0] = sequences,
 * out[1] = frames per sequence, and the maxima over the sequences of out[2] = states, out[3] = arcs, out[4] = unique
 * (frame, pdf) entries, out[5] = states of one time level, out[6] = arcs leaving one level, out[7] = unique entries of one
 * frame; out[8] = LDS bytes of the resident kernel (a whole sequence on chip: 16 * states + 4 * arcs + 4 * unique),
 * out[9] = LDS bytes of the level-windowed kernel (two adjacent levels: 32 * level states + 4 * level arcs + 4 * frame
 * unique), out[10] = bytes of that kernel's log-alpha history (8 per state of the minibatch, in the supervision's device
 * slot), out[11] = the kernel the numerator launches: 0 resident (out[8] <= 160 KB), 1 windowed (otherwise, or with
 * tc_debug_set("force_num_windowed", 1) as it stands at this call), or the negative TC_ERR_* it returns --
 * TC_ERR_UNSUPPORTED when one level does not fit LDS (out[9] + 2 KB > 160 KB) or the history exceeds 4 GiB.
 * End-to-end supervisions have no levels: TC_ERR_INVALID_ARGUMENT, as for a null pointer. */
int tc_supervision_stats(const tc_supervision *supervision, int64_t *out12);

/* Copies the supervision's arc tables to `device` on `stream` (asynchronously: pinned staging; idempotent -- a
 * later call on another stream makes that stream wait for the copy).  The tables live in a slot of a per-device
 * pool: tc_supervision_free returns the slot, and the pool reuses it once the last launch that read it has
 * finished (event query, no synchronisation), so fresh supervisions every minibatch cost no hipMalloc / hipFree
 * after warm-up. */
int tc_supervision_prepare(tc_supervision *supervision, int device, void *stream);
/* The host half of that upload alone -- the tables into the pinned staging of a slot of `device`'s pool -- so that a
 * reader's look-ahead thread can do it ahead of the training thread (tc_rand_reader_set_device); no stream is touched. */
int tc_supervision_stage(tc_supervision *supervision, int device);

/* ---- the hot path -------------------------------------------------------------------------- */

/* Bytes of device scratch the calls below need for this problem size (alpha history etc.; for batches of at most
 * 128 sequences of graphs on the on-chip tied kernel also a second history of the same size: such batches run the
 * forward and the backward recursion of a sequence on two CUs at once -- inside the call, forking to a per-device
 * side stream and joining `stream` again, which HIP-graph capture follows).
 * Sizes, with S sequences, T frames, Hs = graph states rounded up (tied on-chip graphs: to whole planes of 4096):
 *   on-chip graphs          4 (T + 1) S Hs                     the alpha history  (1.27 GB at 256 x 150 x 8192)
 *     tied, Hs <= 8192      + 4 S Hs + ~80 (T + 2) S bytes      one more row, the two-sequence form's normalisers
 *     tied, S <= 128        + 4 (T + 1) S Hs                    the second history of the two-CU form
 *   graphs beyond LDS       4 (T + 1) S' H + 12 S' H + 8 S' P   S' = S rounded up to whole slabs of 16 sequences (32 from
 *                                                              28000 states on): the streamed path's [slab][state][G] matrices
 *                           + 4 T S' P if that is <= 1 GB       exp(y) of every frame, transposed once (else per frame)
 *   tied, 28673..40960 positions  + 8 S (2 Hs + ...)            second half of the gather source, parked row sums (per workgroup)
 * plus a few KB of per-sequence scalars and 4 S (T + 2) bytes of frame sums (used by long utterances only). */
int64_t tc_chain_workspace_bytes(const tc_den_graph *graph, int32_t num_sequences, int32_t frames_per_sequence);

/* Replaces my_lib_ComputeChainObjfAndDeriv (src/my_lib.h:33-42, src/my_lib_chain.cpp:104-136), i.e.
 * [K] chain::ComputeChainObjfAndDeriv:
 *   objf = w*num - w*den;  weight = w*S*T;  l2_term = -0.5*w*l2*sum(y^2)
 *   deriv = w*gamma_num - w*gamma_den - w*l2*y      (written, not accumulated; may be NULL)
 *   xent_deriv = w*gamma_num                        (written when non-NULL)
 * and on NaN/inf or a failed alpha.beta check: deriv = xent_deriv = 0, objf = -10*weight.  Any NaN or +-inf element of
 * nnet_output fails the call, whichever denominator kernel runs and whether or not an arc carries its pdf; so does a finite
 * element whose square overflows float32 (|y| above about 1.8e19): the failure is carried by the sequence's sum of y^2.
 * results_dev3 is DEVICE memory for {objf, l2_term, weight} (the reference writes a CPU
 * THFloatTensor, src/my_lib_chain.cpp:126,130; the host wrapper copies the 12 bytes).
 * Stream capture: this call, tc_chain_objf_and_grad, tc_chain_step and tc_den_forward_backward may be captured in a HIP
 * graph (tested: tests/test_gpu_step.py, tests/test_gpu_tied.py).  Warm the call up once outside the capture (per-device
 * tables, pools and side streams are created on first use).  Inside a capture the supervision's upload becomes a node of
 * the graph -- every replay copies its tables again from the library's pinned block -- and none of the library's events
 * is waited for or recorded on the capturing stream except the fork / join pair of its own side streams; the caller keeps
 * graph, supervision and workspace alive for as long as the graph may be replayed.  (A supervision is new with every
 * minibatch, so a captured TRAINING step is a benchmark's tool; DESIGN.md 7 has what replay saves: host time only.) */
int tc_chain_objf_and_deriv(tc_den_graph *graph, tc_supervision *supervision, const float *nnet_output,
                            int64_t num_rows, int32_t num_cols, int64_t row_stride, float *results_dev3,
                            float *nnet_output_deriv, int64_t deriv_stride, float *xent_output_deriv,
                            int64_t xent_stride, float l2_regularize, float leaky_hmm_coefficient,
                            float xent_regularize, void *workspace, int64_t workspace_bytes, int device,
                            void *stream);

/* The same computation with the outputs in the form the reference's autograd backward returns them
 * (torchain/functions.py:106-115: -mmi_grad for the input, -xent_regularize * xent_grad for xent_input):
 *   grad      = -(w*gamma_num - w*gamma_den - w*l2*y)        xent_grad = -xent_regularize * w*gamma_num
 * so that the wrapper needs no further pass over the matrices (the reference makes one to scale xent_grad and one
 * each to negate).  grad is the exact negative of tc_chain_objf_and_deriv's deriv; results_dev3 is unchanged. */
int tc_chain_objf_and_grad(tc_den_graph *graph, tc_supervision *supervision, const float *nnet_output,
                           int64_t num_rows, int32_t num_cols, int64_t row_stride, float *results_dev3,
                           float *nnet_output_grad, int64_t grad_stride, float *xent_output_grad,
                           int64_t xent_stride, float l2_regularize, float leaky_hmm_coefficient,
                           float xent_regularize, void *workspace, int64_t workspace_bytes, int device,
                           void *stream);

/* ONE call per training step: everything torchain/functions.py:62-115 does around my_lib_ComputeChainObjfAndDeriv --
 * the (B, C, T) -> (T*B, C) copy of `to2d` (functions.py:118-125), the objective, the reference's second call on
 * xent_input when kaldi_way == 0 (functions.py:96-103), the cross-entropy objective, the loss value -objf / weight
 * (functions.py:104) and the matrices in the form and layout backward() returns them (functions.py:106-115).
 *   three_d != 0 : input / xent_input / grad / xent_grad are contiguous (B, C, T) tensors, B = num_sequences of the
 *                  supervision, C = its label_dim, T = its frames_per_sequence;  else 2-D (T*B, C), input and xent_input
 *                  with `row_stride`, grad and xent_grad contiguous.
 *   grad          = -(derivative of the objective w.r.t. input);  xent_grad = -xent_regularize * xent_deriv
 *                   (xent branch: xent_input != NULL and xent_regularize != 0, as in the reference)
 *   results_dev3  : device float[3] {objf, l2_term, weight};  loss_dev1 (nullable): device float[1] = -objf / weight
 *   xent_objf_dev : nullable device double[1] = -xent_regularize * sum(xent_input * xent_deriv) (the sum over xent_grad's
 *                   entries as they are written; the caller divides).  xent_deriv has entries only where the numerator
 *                   has posteriors: a (B, C, T) xent_grad is cleared and those entries written in place, xent_input read
 *                   in place -- no frame-major copies of the two.  kaldi_way == 0: the reference's second call overwrites
 *                   all the first wrote, so only it is made (on xent_input); the objective here is still that of the
 *                   first call's xent_deriv (the numerator alone on `input`)
 *   grad == NULL  : an EVALUATION step (xent_grad must be NULL too): [K] ComputeChainObjfAndDeriv with
 *                   nnet_output_deriv == NULL -- the two forward recursions, results, loss and (when asked for) the
 *                   cross-entropy objective; no backward recursion of the denominator, hence no alpha-beta check (the
 *                   NaN / inf guard on objf stays), nothing written but the scalars.  The reference's validation loop
 *                   (example/chime5/train.py:150-171, under torch.no_grad()) pays for a training step because
 *                   torchain/functions.py:74,82 fill mmi_grad whatever autograd needs.
 * Workspace: tc_chain_step_workspace_bytes(graph, B, T, three_d, xent branch).  No host synchronisation. */
int64_t tc_chain_step_workspace_bytes(const tc_den_graph *graph, int32_t num_sequences, int32_t frames_per_sequence,
                                      int three_d, int with_xent);
int tc_chain_step(tc_den_graph *graph, tc_supervision *supervision, const float *input, const float *xent_input,
                  int three_d, int64_t row_stride, float l2_regularize, float leaky_hmm_coefficient,
                  float xent_regularize, int kaldi_way, float *grad, float *xent_grad, float *results_dev3,
                  float *loss_dev1, double *xent_objf_dev, void *workspace, int64_t workspace_bytes, int device,
                  void *stream);

/* Element types of the tensors of tc_chain_step_typed. */
#define TC_DTYPE_F32 0
#define TC_DTYPE_BF16 1
#define TC_DTYPE_F16 2

/* tc_chain_step on tensors of element type `dtype` (TC_DTYPE_*; anything else: TC_ERR_INVALID_ARGUMENT): input,
 * xent_input, grad and xent_grad are all of that type, in the layouts tc_chain_step takes (2-D grad and xent_grad
 * contiguous).  TC_DTYPE_F32 is tc_chain_step itself, with its workspace.  For bfloat16 / float16 the values are those
 * of tc_chain_step on the same tensors converted to float32 (an exact conversion), with each gradient element rounded
 * once, to nearest even, from that call's float32 value; results_dev3, loss_dev1 and xent_objf_dev stay float32 / float64.
 * Everything between the edges is the float32 computation:
 *   three_d != 0 : the frame-major float32 copy of input (or of xent_input, kaldi_way == 0) that the denominator reads is
 *                  widened from the 16-bit (B, C, T) tensor by the layout copy; the numerator reads the 16-bit tensors
 *                  in place (input or xent_input at its (frame, pdf) pairs, xent_input for the cross-entropy objective)
 *                  and widens in registers.  grad is rounded by the layout copy back, after the scale -1.  xent_grad
 *                  is written into a cleared float32 (B, C, T) scratch and rounded into the caller's tensor in one pass.
 *   three_d == 0 : input (and with the xent branch xent_input), with `row_stride`, are widened into contiguous float32
 *                  matrices in the workspace, and the float32 2-D step runs on them; grad and xent_grad are written
 *                  there in float32 and rounded into the caller's contiguous matrices in one pass each.
 *   soft failure : the float32 scratch is reset as tc_chain_step resets its gradients, and then rounded: a zero gradient
 *                  (-l2 * weight * y with l2 != 0) in the caller's 16-bit tensor.
 * Workspace: tc_chain_step_typed_workspace_bytes(graph, B, T, three_d, xent branch, dtype).  For TC_DTYPE_F32 it equals
 * tc_chain_step_workspace_bytes; for bfloat16 / float16 it adds M = B * T * num_pdfs * 4 bytes (float32 scratch,
 * rounded up to 256 bytes) k times: three_d and the xent branch: k = 1 (the xent gradient); three_d without it: k = 0;
 * 2-D: k = 2 (input and gradient), k = 4 with the xent branch (and xent_input and its gradient). */
int64_t tc_chain_step_typed_workspace_bytes(const tc_den_graph *graph, int32_t num_sequences,
                                            int32_t frames_per_sequence, int three_d, int with_xent, int dtype);
int tc_chain_step_typed(tc_den_graph *graph, tc_supervision *supervision, const void *input, const void *xent_input,
                        int three_d, int64_t row_stride, float l2_regularize, float leaky_hmm_coefficient,
                        float xent_regularize, int kaldi_way, void *grad, void *xent_grad, float *results_dev3,
                        float *loss_dev1, double *xent_objf_dev, int dtype, void *workspace, int64_t workspace_bytes,
                        int device, void *stream);

/* tc_chain_step_typed with Kaldi's per-frame derivative weights ([K] nnet-chain-training.cc: with apply_deriv_weights,
 * nnet_output_deriv.MulRowsVec(deriv_weights) and the same on xent_deriv, after both objectives are formed).
 * deriv_weights: device float32[S * T], 4-byte aligned (else TC_ERR_INVALID_ARGUMENT), one per frame-major row t * S + s
 * (the row order of the 2-D tensors, and of the egs' <DW> / <DW2> weights); NULL is tc_chain_step_typed itself, which is
 * this entry's NULL case.
 *   gradients : every element tc_chain_step_typed writes as g[row, pdf] becomes w[row] * g, one float32 multiply of the
 *               unweighted float32 value; for bfloat16 / float16 that product is rounded once, to nearest even.  This
 *               holds for the MMI gradient, the xent gradient (both kaldi_way settings) and the soft-failure gradient
 *               (-l2 * weight * y, or 0).  So for w >= 0 it is bit for bit the unweighted gradient times w; for w < 0 the
 *               values agree but a zero's sign may differ.
 *   scalars   : results_dev3, loss_dev1 and xent_objf_dev are those of the unweighted call, bit for bit (the cross-entropy
 *               objective sums the unweighted xent_deriv; the weight does not depend on w).
 *   where     : three_d != 0: the layout copy back applies -w[row] in its one multiply (float32 and 16-bit); the xent
 *               entries are weighted as the numerator writes them.  three_d == 0: 16-bit: the rounding pass of the MMI
 *               gradient applies w, the numerator weights the xent entries; float32: the numerator weights the xent
 *               entries, and one in-place pass over the MMI gradient (behind the soft-failure reset) applies w.  The
 *               denominator kernels are not involved.
 *   grad == NULL (an evaluation step): deriv_weights is not read.
 * Workspace: tc_chain_step_typed_workspace_bytes (unchanged).  No host synchronisation; safe under stream capture, where
 * the pointer is baked into the graph and each replay reads the weights' current contents. */
int tc_chain_step_weighted(tc_den_graph *graph, tc_supervision *supervision, const void *input, const void *xent_input,
                           int three_d, int64_t row_stride, float l2_regularize, float leaky_hmm_coefficient,
                           float xent_regularize, int kaldi_way, void *grad, void *xent_grad, float *results_dev3,
                           float *loss_dev1, double *xent_objf_dev, const float *deriv_weights, int dtype, void *workspace,
                           int64_t workspace_bytes, int device, void *stream);

/* tc_chain_step_weighted with an out-of-range penalty on the network output (after [K] PenalizeOutOfRange, restated: the
 * definition below is this library's and is complete).  The denominator kernels take exp(y) at clamp(y, -L, L), L = 30
 * (kOutputLimit), so outside that range an output has lost the objective's restoring force; the penalty gives one back.
 * out_of_range_regularize = c: finite and >= 0, else TC_ERR_INVALID_ARGUMENT; c == 0 is tc_chain_step_weighted itself,
 * which is this entry's c == 0 case (the same kernels and the same launches).
 * With y the float32 value of the CHAIN output `input` (the exact widened value of a 16-bit element; never xent_input, also
 * when kaldi_way == 0 runs the objective on xent_input) and g the float32 MMI gradient element tc_chain_step_typed returns:
 *     p  = y > L ? y - L : (y < -L ? y + L : 0)     one float32 subtract; p = 0 where y is NaN or +-inf
 *     t  = fl32(fl32(2 * c) * p)                     one float32 multiply
 *     g' = fl32(g + t)                               one float32 add, not fused with the multiply
 * which is gradient descent on c * sum (y - clamp(y, -L, L))^2.  Every row of every sequence is penalised (Kaldi takes a
 * random subset of rows and scales up; this is deterministic), and t is not multiplied by the supervision's weight.
 *   order     : deriv_weights apply after, w[row] * g'; a 16-bit gradient is rounded once, from that product.  The penalty
 *               lies behind the soft-failure reset: a failed step returns w[row] * ((l2 * weight * y, or 0) + t).
 *   p == 0    : the element has the bits of the unpenalised call, a zero's sign included.
 *   untouched : results_dev3, loss_dev1, xent_objf_dev and the xent gradient, bit for bit, for both kaldi_way settings: the
 *               penalty is not part of the objective.
 *   where     : three_d != 0, float32 and 16-bit: the layout copy back, which reads `input` at the index it writes.
 *               three_d == 0, 16-bit: the rounding pass of the MMI gradient, which reads the widened float32 input.
 *               three_d == 0, float32: one in-place pass over the MMI gradient that reads `input` with row_stride; it is
 *               the pass that applies deriv_weights when those are given too.  The denominator and the numerator
 *               kernels are not involved.
 *   grad == NULL (an evaluation step): out_of_range_regularize is checked and not used.
 * Workspace: tc_chain_step_typed_workspace_bytes (unchanged, every layout and dtype).  No host synchronisation; safe under
 * stream capture. */
int tc_chain_step_penalized(tc_den_graph *graph, tc_supervision *supervision, const void *input, const void *xent_input,
                            int three_d, int64_t row_stride, float l2_regularize, float leaky_hmm_coefficient,
                            float xent_regularize, int kaldi_way, void *grad, void *xent_grad, float *results_dev3,
                            float *loss_dev1, double *xent_objf_dev, const float *deriv_weights,
                            float out_of_range_regularize, int dtype, void *workspace, int64_t workspace_bytes, int device,
                            void *stream);

/* Layouts of the tensors of tc_chain_step_strided. */
#define TC_LAYOUT_ROWS 0         /* 2-D frame-major (T*B, C) with row_stride: three_d == 0 of the entries above */
#define TC_LAYOUT_BCT 1          /* contiguous (B, C, T), the reference's 3-D input: three_d != 0 */
#define TC_LAYOUT_CHANNEL_LAST 2 /* a (B, C, T) view with channel stride 1: element (b, c, t) at b*batch_stride + t*frame_stride + c */

/* tc_chain_step_penalized with a layout code in place of three_d, for network outputs that come with their channels last.
 * The reference's contract is "3-D input is (B, C, T)" (torchain/functions.py:118-125 permutes it to frame-major rows
 * t*B + b); a batch-first LSTM or Transformer produces (B, T, C) and its user passes out.transpose(1, 2), each half of a
 * joint chain / xent head is a strided slice out[..., :P] / out[..., P:] of such a tensor.  Those views are
 * TC_LAYOUT_CHANNEL_LAST: no copy is made contiguous first.
 *   layout 0, 1 : tc_chain_step_penalized with three_d = layout, argument for argument; batch_stride and frame_stride are
 *                 not read.
 *   layout 2    : batch_stride / frame_stride are ELEMENT strides shared by input and xent_input; row_stride is not read.
 *                 The stride of a dimension of size 1 is ignored.  Otherwise each must be >= num_pdfs and the B * T rows must
 *                 not overlap: batch_stride >= (T-1)*frame_stride + C (batch-major) or frame_stride >= (B-1)*batch_stride + C
 *                 (time-major); anything else -- negative, zero, interleaved -- is TC_ERR_INVALID_ARGUMENT, as is a pointer
 *                 that is not a multiple of the element size, and nothing is written.
 *                 grad and xent_grad are DENSE (B, T, C) tensors of `dtype`: element (b, c, t) at (b*T + t)*C + c.
 *   values      : those of tc_chain_step_penalized with three_d != 0 on the contiguous (B, C, T) copy of the same values, bit
 *                 for bit, for every dtype and option: results_dev3, loss_dev1, xent_objf_dev and every gradient element.
 *                 One exception, TC_DTYPE_F16 without weights and penalty: where the float32 MMI gradient is exactly +-0 the
 *                 two may differ in the zero's sign.  Here the float16 element is the rounded float32 value -1 * g on every
 *                 path; the (B, C, T) copy back fuses the product into the conversion on some of its paths (v_fma_mixlo_f16,
 *                 whose + 0 addend turns -0 into +0).  Equal values everywhere.
 *   how         : one gather per input (rows b*batch_stride + t*frame_stride -> contiguous float32 frame-major rows, widened
 *                 exactly), the float32 2-D computation on those, one scatter per gradient.  The MMI gradient's scatter applies
 *                 what the (B, C, T) copy back applies, in its order: scale -1; with deriv_weights (-1 * w[row]) * g in one
 *                 multiply; with the penalty w[row] * (-g + t), reading `input` at the row it writes; one rounding for 16-bit
 *                 tensors.  It runs behind the soft-failure reset.  The xent gradient's entries are scaled and weighted by
 *                 the numerator in float32 and only moved (and, for 16 bits, rounded once) by their scatter; the cross-entropy
 *                 objective sums the unweighted entries.
 *   scratch     : a float32 step keeps the frame-major xent gradient in the caller's `grad` until the MMI gradient's scatter
 *                 overwrites it: `grad` and `xent_grad` must be distinct, and neither holds anything else meanwhile.
 *   grad == NULL: the evaluation step, as in the other entries; the gathers only.
 * Workspace: tc_chain_step_strided_workspace_bytes(graph, B, T, layout, xent branch, dtype); for layout 2 it equals that of
 * layout 1.  No host synchronisation, nothing allocated; safe under stream capture.  tc_debug_counter("channel_last_steps")
 * counts the steps taken in layout 2; their gathers and scatters count as "layout_launches". */
int64_t tc_chain_step_strided_workspace_bytes(const tc_den_graph *graph, int32_t num_sequences,
                                              int32_t frames_per_sequence, int layout, int with_xent, int dtype);
int tc_chain_step_strided(tc_den_graph *graph, tc_supervision *supervision, const void *input, const void *xent_input,
                          int layout, int64_t row_stride, int64_t batch_stride, int64_t frame_stride, float l2_regularize,
                          float leaky_hmm_coefficient, float xent_regularize, int kaldi_way, void *grad, void *xent_grad,
                          float *results_dev3, float *loss_dev1, double *xent_objf_dev, const float *deriv_weights,
                          float out_of_range_regularize, int dtype, void *workspace, int64_t workspace_bytes, int device,
                          void *stream);

/* tc_chain_step_strided with the sequences' own objectives reported, and with a minibatch that survives a failed sequence.
 * The reference (and Kaldi, whose egs are filtered offline) gives up the whole minibatch when its objective is not finite:
 * objf = -10 * weight, every gradient reset (src/my_lib_chain.cpp:104-136 -> [K] ComputeChainObjfAndDeriv).  A ragged
 * minibatch built from whole utterances meets such sequences -- an end-to-end FST with no path of exactly T_s arcs, a NaN
 * or inf in one sequence's activations -- and its caller cannot tell which one it was.
 *   seq_results_dev  : nullable; device double[num_sequences][6], 8-byte aligned, one row per sequence:
 *                      {num_logprob, den_logprob, sum_y2, xent_sum, frames, status}.  The two log-probabilities are the
 *                      unweighted ones (the sequence's objective is weight * (num_logprob - den_logprob)); xent_sum is the
 *                      sequence's share of xent_objf_dev, scaled as that is, 0 without the xent branch; frames is its own
 *                      T_s; status is a bit set, 0 for ok: 1 numerator non-finite (no path: -inf; forward and backward
 *                      totals that disagree: NaN; a non-finite cross-entropy sum, which is made of the numerator's
 *                      posteriors), 2 denominator non-finite (its log-probability or sum y^2: a NaN or inf among the
 *                      sequence's activations), 4 an alpha-beta check value non-finite (only when grad != NULL).
 *                      Written whatever isolate_failures says; every other output is then tc_chain_step_strided's, bit
 *                      for bit.
 *   isolate_failures : != 0: a sequence FAILED when its status is not 0 -- no tolerance is involved.  Then
 *                      results_dev3 = {objf, l2_term, weight}, loss_dev1 and xent_objf_dev are formed from the surviving
 *                      sequences alone, summed in the order of the unmasked call (a failed sequence's term is an exact
 *                      +0.0): weight = supervision weight * (the survivors' frames), loss = -objf / weight, and Kaldi's
 *                      alpha-beta check |sum - S| > 2 is held against the survivors' sums and their count.  Every
 *                      gradient element of a failed sequence, in grad and in xent_grad, is +0 in every layout and dtype,
 *                      as a ragged minibatch's padding is: no l2 term, no penalty, no deriv_weights product -- a failed
 *                      sequence is a sequence of no frames.  The other sequences' elements are the bits of the call
 *                      without the switch.
 *                      Nothing failed: every output is that call's, bit for bit.  Every sequence failed, or the
 *                      survivors miss the alpha-beta check: the whole minibatch takes the failure route exactly as without
 *                      the switch (status still tells the sequences apart).
 *                      Whether a non-finite sequence can make its NEIGHBOURS non-finite (they are then reported as
 *                      failed too, by the same rule) depends on the denominator kernel: DESIGN.md 4.13 lists the families.
 *   how              : a sibling of the scalar epilogue forms the statuses and both sets of sums and leaves each
 *                      sequence's surviving frames beside the failure flag in the workspace; with isolate_failures the
 *                      ragged minibatches' padding pass runs on those, last of all (one more launch per gradient for a
 *                      uniform supervision, none for a ragged one).  The denominator and numerator kernels are untouched.
 *   grad == NULL     : the evaluation step with the same scalars; nothing else is written.
 * isolate_failures == 0 and seq_results_dev == NULL: tc_chain_step_strided, launch for launch.  Same workspace.  No host
 * synchronisation, nothing allocated; safe under stream capture.  The split entries (tc_chain_objf_and_deriv,
 * tc_chain_objf_and_grad, tc_den_forward_backward*) do not take the switch. */
int tc_chain_step_per_sequence(tc_den_graph *graph, tc_supervision *supervision, const void *input, const void *xent_input,
                               int layout, int64_t row_stride, int64_t batch_stride, int64_t frame_stride,
                               float l2_regularize, float leaky_hmm_coefficient, float xent_regularize, int kaldi_way,
                               void *grad, void *xent_grad, float *results_dev3, float *loss_dev1, double *xent_objf_dev,
                               const float *deriv_weights, float out_of_range_regularize, int dtype, void *workspace,
                               int64_t workspace_bytes, int device, void *stream, int isolate_failures,
                               double *seq_results_dev);

/* tc_chain_step_per_sequence with the cross-entropy head's log-softmax folded in.
 * Kaldi's chain recipes end the cross-entropy head in a log-softmax (the "output-xent" layer).  The trainer takes
 * xent_objf = sum(xent_output * xent_deriv) on its LOG-PROBABILITIES and back-propagates xent_regularize * xent_deriv (after
 * MulRowsVec by deriv_weights) THROUGH that log-softmax ([K] nnet-chain-training.cc).  The reference has no log-softmax in
 * training: its head ends in a plain Conv1d, torchain/functions.py:88-89 carries a "TODO: compute xent loss like kaldi?",
 * and only forward.py:67 applies log_softmax, at inference.  Without the switch the step mirrors the reference: xent_grad is
 * V = -xent_regularize * deriv_weights[row] * weight * gamma_num, the gradient of an objective linear in xent_input.
 *   xent_log_softmax : != 0, with the xent branch active (xent_input given, xent_regularize != 0), x = xent_input, row =
 *                      one (sequence, frame), c = channel, everything in float32 from the widened input:
 *                        mx = max_c x[row, c],  ls = log(sum_c exp(x[row, c] - mx))            (lse = mx + ls)
 *                        (float32 exponentials, their sum carried in double and its logarithm rounded once)
 *                        xent_grad[row, c] = V[row, c] - (sum_c' V[row, c']) * exp((x[row, c] - mx) - ls)
 *                      rounded once for 16-bit tensors; the gradient is dense.  A row of V without a non-zero entry -- a
 *                      ragged minibatch's padding, a frame of deriv_weights == 0, a failed sequence of isolate_failures,
 *                      the whole minibatch on the soft-failure route -- is +0, chosen by a select: a NaN in x there does
 *                      not reach the gradient.
 *                      xent_objf_dev = (-xent_regularize) * sum_rows sum_c weight * gamma_num * ((x - mx) - ls), the
 *                      subtractions made in double, summed in double in the order of the call without the switch; the
 *                      xent_sum of seq_results_dev and the survivors' sum of isolate_failures carry the same term.  The
 *                      objective ignores deriv_weights, as without the switch.
 *                      A NaN or +-inf in a live row of xent_input makes every element of that row's gradient and the
 *                      row's objective term non-finite (a sequence's xent_sum with it, and its status bit 1); other rows
 *                      keep their bits.
 *                      results_dev3, loss_dev1, grad and every value formed from `input` do not change by a bit.
 *                      kaldi_way == 0 with the switch: TC_ERR_INVALID_ARGUMENT (the whole objective is then run again on
 *                      xent_input, which is another question).  Without the xent branch the switch does nothing.
 *   how              : two launches of xent_softmax_kernels.hip.  The row statistics (mx, ls), 2 floats a row in the
 *                      workspace, are formed in front of the objective from xent_input where the step reads it (float32
 *                      rows, the widened / gathered float32 scratch, or the caller's (B, C, T) tensor of `dtype`); the
 *                      numerator kernels subtract them in their cross-entropy sums.  The gradient pass runs behind the
 *                      objective's soft-failure reset and in front of the last passes, in place on the float32 matrix the
 *                      numerator wrote V to.  tc_debug_counter("xent_log_softmax_launches") counts both.
 *   grad == NULL     : the evaluation step returns the same xent_objf_dev (statistics launch only) and writes no gradient.
 * xent_log_softmax == 0: tc_chain_step_per_sequence, launch for launch, and its workspace suffices.
 * Workspace: tc_chain_step_log_softmax_workspace_bytes = tc_chain_step_strided_workspace_bytes plus, with the xent branch,
 * the row statistics (8 * num_sequences * frames_per_sequence bytes, rounded up to 256).  No host synchronisation, nothing
 * allocated; safe under stream capture.  The split entries and the torch.library operator do not take the switch. */
int64_t tc_chain_step_log_softmax_workspace_bytes(const tc_den_graph *graph, int32_t num_sequences,
                                                  int32_t frames_per_sequence, int layout, int with_xent, int dtype);
int tc_chain_step_log_softmax(tc_den_graph *graph, tc_supervision *supervision, const void *input, const void *xent_input,
                              int layout, int64_t row_stride, int64_t batch_stride, int64_t frame_stride,
                              float l2_regularize, float leaky_hmm_coefficient, float xent_regularize, int kaldi_way,
                              void *grad, void *xent_grad, float *results_dev3, float *loss_dev1, double *xent_objf_dev,
                              const float *deriv_weights, float out_of_range_regularize, int dtype, void *workspace,
                              int64_t workspace_bytes, int device, void *stream, int isolate_failures,
                              double *seq_results_dev, int xent_log_softmax);

/* Boosted LF-MMI (bMMI; Povey et al. 2008, the lattice-free form of [K]'s discriminative --boost): tc_chain_step_log_softmax
 * with an accuracy margin on the denominator.  Every denominator path's weight is multiplied by exp(-boost * A(path)), A the
 * path's frame accuracy against a reference, so a competitor must be beaten by a margin that grows with its error.  Frame
 * accuracy is additive over frames: the boost is a shift of the DENOMINATOR'S input alone.
 *   a_t(j)    : exactly tc_den_expected_accuracy's.  Hard form: ref_pdfs_dev, device int32[S * T], entry s * T + t;
 *               a = 1 iff 0 <= ref_t < P and class(j) == class(ref_t), else 0 (-1 or any out-of-range entry: the frame scores
 *               nothing); pdf_class_dev NULL (identity) or device int32[P].  Dense form: accuracy, device float32 (T*S, P),
 *               row t*S + s, rows accuracy_row_stride >= P floats apart, any finite values.  Exactly one of ref_pdfs_dev /
 *               accuracy is given; pdf_class_dev goes with ref_pdfs_dev only.  Both are constants: no gradient flows into them.
 *   y_b       : float32 with two roundings.  y32 the input widened exactly, b32 = boost:
 *                   y_b = fl32(y32 - fl32(b32 * a))            (__fmul_rn, __fsub_rn: never one FMA)
 *               The hard form is the dense form on the float32 indicator.
 *   who sees it : the denominator alone runs on y_b, with its usual clamp of exp() at +-30 applied to y_b.  The numerator, the
 *               l2 term and its gradient -l2 * weight * y, the out-of-range penalty, deriv_weights and the cross-entropy
 *               branch act on the true y:
 *                   objf = weight * (num_logprob(y) - den_logprob(y_b))
 *                   grad = weight * (gamma_num(y) - gamma_den(y_b)) - l2 * weight * y, then penalty and row weights.
 *               results_dev3, loss_dev1, xent_objf_dev and seq_results_dev keep their layout; den_logprob is the boosted
 *               denominator's.  The objective is no longer bounded by 0: for a in [0, 1] and boost >= 0 on a composed
 *               supervision it is bounded by weight * boost * sum_s T_s.
 *   edges     : boost must be finite (negative allowed); a ragged handle's entries and rows of frames t >= T_s are never read
 *               and its padding gradients are +0; a non-finite accuracy value in a sequence's valid frames behaves as a
 *               non-finite network output there would (the soft failure of the minibatch, or of that sequence alone with
 *               isolate_failures); grad == NULL is the boosted evaluation step.  kaldi_way == 0 with the xent branch active:
 *               TC_ERR_INVALID_ARGUMENT, as xent_log_softmax.  TC_ERR_INVALID_ARGUMENT also for a boost that is not finite,
 *               both or neither reference, classes without ref_pdfs_dev, pointers not 4-byte aligned, accuracy_row_stride < P.
 *               Callers send boost == 0 to tc_chain_step_log_softmax: this entry runs its passes whatever the value.
 *   how       : one streaming pass (boost_kernels.hip) forms y_b, frame-major float32, from the caller's tensor where it lies
 *               -- in place of the plain copy of a (B, C, T) step, beside the gather / widening of the others -- in front of
 *               the denominator.  The denominator kernels fold the l2 term of the matrix they read into their passes; with
 *               l2_regularize != 0 two small launches put it back on the true y: sum(y^2) = sum(y_b^2) + sum(2 y_b d + d^2)
 *               per sequence (doubles, fixed order) and grad -= l2_scale * d, d = fl32(b32 * a), over the elements with
 *               d != 0 (S * T of them for a hard reference without classes).  tc_debug_counter("boost_launches") counts all.
 * Workspace: tc_chain_step_boosted_workspace_bytes = tc_chain_step_log_softmax_workspace_bytes plus, for every layout but
 * TC_LAYOUT_BCT, one more num_sequences * frames_per_sequence * P float32 matrix (rounded up to 256 bytes): a 2-D or
 * channel-last step keeps the true y where the numerator reads it.  No host synchronisation, nothing allocated; the reference
 * and the accuracy are read where they lie, so a captured step replays on their current values.  The split entries and the
 * torch.library operator do not take the option. */
int64_t tc_chain_step_boosted_workspace_bytes(const tc_den_graph *graph, int32_t num_sequences, int32_t frames_per_sequence,
                                              int layout, int with_xent, int dtype);
int tc_chain_step_boosted(tc_den_graph *graph, tc_supervision *supervision, const void *input, const void *xent_input,
                          int layout, int64_t row_stride, int64_t batch_stride, int64_t frame_stride, float l2_regularize,
                          float leaky_hmm_coefficient, float xent_regularize, int kaldi_way, void *grad, void *xent_grad,
                          float *results_dev3, float *loss_dev1, double *xent_objf_dev, const float *deriv_weights,
                          float out_of_range_regularize, int dtype, void *workspace, int64_t workspace_bytes, int device,
                          void *stream, int isolate_failures, double *seq_results_dev, int xent_log_softmax, float boost,
                          const int32_t *ref_pdfs_dev /* [S * T] or NULL */, const int32_t *pdf_class_dev /* nullable, [P] */,
                          const float *accuracy /* (T*S, P) or NULL */, int64_t accuracy_row_stride);

/* The boost pass alone: out2d[(t*S + s) * out_stride + c] = fl32(y32 - fl32(boost * a_t(c))), y32 element (s, c, t) of
 * `input` widened -- TC_LAYOUT_ROWS (row t*S + s at row_stride elements), TC_LAYOUT_BCT (contiguous (S, C, T)) or
 * TC_LAYOUT_CHANNEL_LAST (element at s * batch_stride + t * frame_stride + c), float32 / bfloat16 / float16.  a_t, boost and
 * their checks are tc_chain_step_boosted's.  seq_frames_dev: NULL or device int32[S], the lengths T_s (held to 1 .. T): rows
 * of frames t >= T_s read neither the reference nor the accuracy and receive the widened input.  16-byte accesses where
 * every address allows them, scalar tails elsewhere; rows are addressed in 64 bits.  One launch, asynchronous on `stream`,
 * counted in "boost_launches".  TC_ERR_UNSUPPORTED: a (B, C, T) shape beyond tc_to2d's grid. */
int tc_boost_rows(const void *input, int dtype, int layout, int32_t S, int32_t C, int32_t T, int64_t row_stride,
                  int64_t batch_stride, int64_t frame_stride, const int32_t *seq_frames_dev /* nullable */, float boost,
                  const int32_t *ref_pdfs_dev /* [S * T] or NULL */, const int32_t *pdf_class_dev /* nullable, [C] */,
                  const float *accuracy /* (T*S, C) or NULL */, int64_t accuracy_row_stride, float *out2d, int64_t out_stride,
                  int device, void *stream);

/* The benchmarked unit: [K] DenominatorComputation::Forward() + Backward(deriv_weight, deriv)
 * (direct use in the reference: src/chain-supervision-test.hpp:403-414).
 *   logprob_dev   : device double[1], sum over sequences of the denominator log-prob
 *   deriv         : nullable; accumulate != 0 -> deriv += deriv_weight*gamma (Kaldi's semantics),
 *                   accumulate == 0 -> deriv  = deriv_weight*gamma - l2_scale*y (one store per element)
 *   status_dev    : nullable device int32[1], set to 0 when the t=0 checks pass, else nonzero
 */
int tc_den_forward_backward(tc_den_graph *graph, int32_t num_sequences, const float *nnet_output,
                            int64_t num_rows, int32_t num_cols, int64_t row_stride,
                            float leaky_hmm_coefficient, float deriv_weight, float l2_scale, int accumulate,
                            float *deriv, int64_t deriv_stride, double *logprob_dev, int32_t *status_dev,
                            void *workspace, int64_t workspace_bytes, int device, void *stream);

/* tc_den_forward_backward on a ragged batch: seq_frames_dev[s] (DEVICE memory, int32, num_sequences entries, 4-byte
 * aligned) frames of sequence s, max_frames the longest and num_rows == max_frames * num_sequences.  A sequence reads and
 * writes rows t * num_sequences + s of its own frames only; with accumulate == 0 the derivative's padding rows are +0,
 * with accumulate != 0 they are not touched.  Entries outside 1 .. max_frames are taken as the nearer bound.  logprob_dev:
 * the sum of the sequences' log-probs over their own frames.  The workspace is tc_chain_workspace_bytes(graph,
 * num_sequences, max_frames).  The kernel is the graph class's one-workgroup-per-sequence form, whatever the launch
 * switches, for fewer than 8 sequences, for more than half the device's CUs, without a derivative and on general graphs;
 * a tied graph's batch in between takes two workgroups per sequence, each sequence meeting at half its own length, unless
 * "no_mitm" or "no_phase_split" is set (the lengths are read on the device only: a sequence of one frame is run by one
 * of its two workgroups alone).  TC_ERR_UNSUPPORTED for a graph on the streamed path (nothing is launched or written). */
int tc_den_forward_backward_ragged(tc_den_graph *graph, int32_t num_sequences, const float *nnet_output,
                                   int64_t num_rows, int32_t num_cols, int64_t row_stride,
                                   float leaky_hmm_coefficient, float deriv_weight, float l2_scale, int accumulate,
                                   float *deriv, int64_t deriv_stride, const int32_t *seq_frames_dev, int32_t max_frames,
                                   double *logprob_dev, int32_t *status_dev, void *workspace, int64_t workspace_bytes,
                                   int device, void *stream);

/* [K] NumeratorComputation::Forward() + Backward() (src/chain-supervision-test.hpp:99-107):
 *   logprob_dev : device double[1] = weight * log Z_num
 *   deriv       : nullable; deriv[row, pdf] += weight * occupation at the supervision's (row, pdf)s */
int tc_num_forward_backward(tc_supervision *supervision, const float *nnet_output, int64_t num_rows,
                            int32_t num_cols, int64_t row_stride, float *deriv, int64_t deriv_stride,
                            double *logprob_dev, void *workspace, int64_t workspace_bytes, int device,
                            void *stream);

/* The single most likely path of every sequence of a supervision under the network's outputs: the frame-level pdf
 * alignment ([K] gets it from a CPU decoder, one utterance at a time; a flat-start recipe builds its regular chain model
 * from it, and frame accuracies are counted against it).  Regular and end-to-end handles, uniform and ragged.
 *   nnet_output : layout_bct == 0: the 2-D float32 matrix (T*S, P), row t*S + s, rows row_stride floats apart (dtype must
 *                 be TC_DTYPE_F32); layout_bct != 0: the contiguous (S, P, T) tensor of `dtype` (TC_DTYPE_*; row_stride is
 *                 not read).  num_rows == S * T and num_cols == P of the handle, T the longest sequence's.
 *   pdf_dev     : device int32[S * T]; entry s * T + t is the pdf (0-based: ilabel - 1) of frame t of sequence s, -1 in
 *                 the padding frames t >= T_s of a ragged handle
 *   score_dev   : device double[S]: the path's log score, the sum of y_t(pdf_t) - arc cost along the path minus the final
 *                 cost.  The supervision's weight does not enter.
 * A sequence with no path of exactly T_s arcs to a final state gets score -inf and -1 in all its frames; the other
 * sequences are unaffected.  Nothing at frames >= T_s is read.  Among paths of exactly equal score one is returned, the
 * same one at every call.
 * Arithmetic: the numerator's forward recursion with max in place of the log-sum -- each y + (-cost) is one float32 sum,
 * everything else is double -- so the score is within T_s * 2^-23 * max(|y| + |cost|) of the path's float64 score.
 * One launch (num_best_path_kernels.hip): one workgroup per sequence walks the frames with two adjacent levels (regular)
 * or two score vectors (end-to-end) in LDS and leaves every state's score in the supervision's pool slot -- the history
 * the numerator kernels use, which is scratch: a later objective call on the handle gives the bits it gives without
 * this call -- then one wavefront traces back from the best final state.  A regular supervision needs
 * 16 * L + 4 * U + 2048 <= 163840 bytes of LDS, L the widest time level's states (rounded up to 2) and U the most unique
 * (frame, pdf) entries of one frame (rounded up to 4): about 8000 states a level when each has a pdf of its own, where
 * the level-windowed numerator needs 32 * L + 4 * U + 4 * (arcs leaving a level); beyond that TC_ERR_UNSUPPORTED.  End-to-end supervisions:
 * 16 * ceil4(states) + 4 * ceil4(distinct pdfs) bytes for the two score vectors and the frame's y of one sequence, laid out
 * per sequence (the kernel has no other LDS): every sequence of a handle of tc_supervision_create_e2e, _e2e_ragged and
 * _e2e_any meets it, so no end-to-end handle is refused on size.
 * TC_ERR_INVALID_ARGUMENT, before any device call: a null pointer, num_rows or num_cols that are not the handle's, an
 * unknown dtype, a 2-D call with a 16-bit dtype or row_stride < num_cols.  Asynchronous on `stream`; no workspace, and
 * nothing is allocated once the supervision is staged.  tc_debug_counter("best_path_launches") counts the launches. */
int tc_supervision_best_path(tc_supervision *supervision, const void *nnet_output, int dtype, int layout_bct,
                             int64_t num_rows, int32_t num_cols, int64_t row_stride, int32_t *pdf_dev, double *score_dev,
                             int device, void *stream);

/* The single strongest path through the DENOMINATOR graph under the network's outputs: a phone-LM-constrained free decoding
 * of every sequence of a minibatch (the numerator's counterpart is tc_supervision_best_path above; [K] has neither on the
 * GPU).  The score of a path of states h_0 .. h_T joined by arcs a_1 .. a_T is
 *     log pi(h_0) + sum_{t = 1 .. T} ( log w(a_t) + y_{t-1}(pdf(a_t)) )
 * with pi the graph's initial probabilities (tc_den_graph_initial_probs: the ones the denominator uses; a state with
 * pi == 0 starts no path) and every state final at cost 0, as in [K]'s denominator computation.  y is taken as it is, not
 * clamped.  The leaky-HMM coefficient does not enter: it smooths a sum and is not a path.
 *   S, nnet_output, dtype, layout_bct, num_rows, num_cols, row_stride : as tc_supervision_best_path's -- the 2-D float32
 *                 matrix (T*S, P), row t*S + s, rows row_stride floats apart, or (layout_bct != 0) the contiguous (S, P, T)
 *                 tensor of `dtype`; num_rows == S * max_frames, num_cols == the graph's pdfs.
 *   seq_frames_dev : device int32[S], the sequences' lengths T_s (held to 1 .. max_frames), or NULL: max_frames each.
 *                 Nothing at frames t >= T_s is read.
 *   pdf_dev     : device int32[S * T], entry s * T + t the 0-based pdf of frame t, -1 in the padding frames t >= T_s
 *   state_dev   : NULL, or device int32[S * (T + 1)], entry s * (T + 1) + t the state h_t of the FST, -1 for t > T_s
 *   score_dev   : device double[S]
 * Arithmetic: log w and log pi are float64 logarithms rounded to float32 once on the host; log w + y is one float32 sum; the
 * running score is float32, one add and one max per arc.  A returned score is therefore within T_s * 2^-23 * M of the
 * float64 score of the path that is returned, M the largest running |score| along that path, and no returned score is
 * lower than the float64 optimum by more than the same bound.  Among paths of exactly equal score one is returned: the
 * same one at every call, whatever the sequence's place in the batch and whatever the other sequences are (the lowest last
 * state, then at every frame the in-arc that comes first in the graph's arc list).
 * A sequence with a NaN or +-inf anywhere in the rows of its valid frames (any pdf) gets score NaN and -1 in all its
 * slots; one without a path of T_s arcs gets -inf and -1s; the other sequences keep their bits.
 * One launch (den_best_path_kernels.hip), one workgroup per sequence: a (max, +) forward pass over a CSR by destination
 * state of the FST's own arcs (built from the graph on the first call per device, in device memory of its own: the
 * tables of the training step are not touched, and a step on the graph gives the same bits before and after), every
 * state's score to the workspace, then a traceback by one wavefront that finds each maximum again bit for bit from those
 * scores -- no back-pointers.  Workspace: (T + 1) * Hs * 4 bytes per sequence, Hs the graph's states rounded up to 4 (the
 * whole rounded up to 256), 16-byte aligned.  The previous frame's scores are kept in LDS while 8 * Hs + 1024 <= 163840
 * (20352 states); larger graphs read them from the history row just written ("den_best_path_streamed_launches" counts
 * those launches, tc_debug_set("force_den_best_path_streamed", 1) sends every graph that way).  Graphs of every size.
 * TC_ERR_INVALID_ARGUMENT, before any device call: a null pointer, S or max_frames <= 0, num_rows != S * max_frames,
 * num_cols that are not the graph's, an unknown dtype, a 2-D call with a 16-bit dtype or row_stride < num_cols, lengths
 * that are not 4-byte aligned.  TC_ERR_WORKSPACE: a workspace that is null, too small or not 16-byte aligned.
 * Asynchronous on `stream`; nothing is allocated after the graph's first call on the device.
 * tc_debug_counter("den_best_path_launches") counts the launches; "den_launches" does not move. */
int64_t tc_den_best_path_workspace_bytes(const tc_den_graph *g, int32_t S, int32_t T);
int tc_den_best_path(tc_den_graph *g, int32_t S, const void *nnet_output, int dtype, int layout_bct, int64_t num_rows,
                     int32_t num_cols, int64_t row_stride, const int32_t *seq_frames_dev /* nullable: T each */,
                     int32_t max_frames, int32_t *pdf_dev /* [S * T] */, int32_t *state_dev /* nullable, [S * (T + 1)] */,
                     double *score_dev /* [S] */, void *workspace, int64_t workspace_bytes, int device, void *stream);

/* The expected frame accuracy of the DENOMINATOR graph's paths against a frame-level reference, and its gradient: the
 * lattice-free sMBR criterion (Kanda et al. 2018), the step [K] takes after chain training with a decoder and lattices
 * (run_discriminative.sh) and this library takes on den.fst alone.  Per sequence
 *     E_s[A] = sum_paths P(path | y_s) * sum_t a_t(pdf_t(path))
 * under the denominator's own model -- p_t(j) = exp(clamp(y_t(j), +-30)), the graph's initial probabilities, the leaky-HMM
 * coefficient, every state final -- with a_t(j) = 1 where 0 <= ref_t < P and class(j) == class(ref_t), else 0.
 *   S, nnet_output, num_rows, num_cols, row_stride : the 2-D float32 matrix (T*S, P), row t*S + s, rows row_stride floats
 *                 apart; num_rows == S * max_frames, num_cols == the graph's pdfs.  (The C entries take this layout only.)
 *   seq_frames_dev : device int32[S], the sequences' lengths T_s (held to 1 .. max_frames), or NULL: max_frames each.
 *   ref_dev     : device int32[S * T], entry s * T + t the 0-based reference pdf of frame t (the layout tc_den_best_path
 *                 and tc_supervision_best_path write).  A value outside 0 .. P-1 in a valid frame: the frame scores
 *                 nothing (silence, say).  Padding entries are not read.
 *   class_dev   : NULL (identity: state-level sMBR), or device int32[P], a map of the pdfs to classes of any values -- a
 *                 pdf -> phone map gives an MPFE-style criterion.
 * tc_den_expected_accuracy: the value.
 *   gamma       : device float32 (T*S, P), rows gamma_stride floats apart: scratch that holds, on return, the DENOMINATOR
 *                 POSTERIORS gamma_t(j) of the batch -- a by-product callers may use.  The entry runs
 *                 tc_den_forward_backward (with lengths: tc_den_forward_backward_ragged) into it, deriv_weight 1, l2_scale
 *                 0, accumulate 0, by whatever kernel the graph's class takes; a ragged batch's padding rows are +0.
 *   frame_acc_dev : device float32[S * T], entry s * T + t the frame's expected accuracy m_t = sum_j gamma_t(j) a_t(j),
 *                 summed in double (a lane's pdfs in order, then a butterfly over the wave); 0 in padding frames.
 *   acc_dev     : device double[S], E_s = sum_t m_t, a double sum of those float32 values in frame order.
 *   One further launch (den_accuracy_kernels.hip), one workgroup per sequence.  It also looks at every nnet_output element
 *   of the sequence's valid frames, as tc_den_best_path does: a sequence with a NaN or +-inf there gets acc NaN (and NaN in
 *   its valid frames of frame_acc_dev); the other sequences keep their bits.
 *   Workspace: tc_den_expected_accuracy_workspace_bytes == tc_chain_workspace_bytes.
 *   TC_ERR_UNSUPPORTED, passed through: lengths on a graph of the streamed path.
 * tc_den_expected_accuracy_grad: grad[t*S + s, :] = seq_scale[s] * dE_s / dy_t, overwritten, one store per element
 * (seq_scale_dev: NULL or device float32[S]; NULL: 1).  Padding rows, and every row of a sequence with a NaN or +-inf in its
 * valid frames, are exactly +0.  Every row sums to 0 up to rounding.
 *   frame_acc_dev : what tc_den_expected_accuracy left.  The kernel subtracts m_t from a_t: the gradient does not depend
 *                 on these constants, its float32 arithmetic does (without them it is the small difference of terms of
 *                 the size of E[A]).
 *   One launch (den_accuracy_kernels.hip, whose header states the recursions), one workgroup per sequence: a forward pass
 *   that carries the accuracy mass beside alpha, a backward pass that carries it beside beta and forms the gradient pdf by
 *   pdf, over three CSRs of the FST's own arcs (by destination, by source, by pdf; built from the graph on the first call
 *   per device, in device memory of their own: the tables of the training step are not touched, and a step on the graph
 *   gives the same bits before and after).  Vectors are float32, every sum over arcs or states is a double.  No atomics and
 *   fixed orders: a sequence's bits depend neither on the call, nor on its place in the batch, nor on the other sequences.
 *   Workspace (tc_den_expected_accuracy_grad_workspace_bytes), per sequence, Hs and Ps the graph's states and pdfs rounded
 *   up to 4: alpha'_t and A'_t of every frame, 2 * (T + 1) * Hs floats; 1 / asum_t, T + 1 floats rounded up to 4; and
 *   4 * Hs + 2 * Ps floats for the per-frame vectors; the whole rounded up to 256 bytes, 16-byte aligned.
 *   The per-frame vectors -- four by state, two by pdf -- stay in LDS while 16 * Hs + 8 * Ps + 1024 <= 163840 bytes (for
 *   instance 8192 states with 3968 pdfs); beyond that the same code keeps them in the workspace, with the same bits
 *   ("den_accuracy_grad_streamed_launches" counts those launches, tc_debug_set("force_den_accuracy_streamed", 1) sends
 *   every graph that way).  Graphs of every size, lengths on every graph.
 * Both: TC_ERR_INVALID_ARGUMENT, before any device call: a null pointer (class_dev, seq_frames_dev and seq_scale_dev may
 * be null), S or max_frames <= 0, num_rows != S * max_frames, num_cols that are not the graph's, a row, gamma or grad stride
 * below num_cols, a leaky-HMM coefficient that is negative or not finite, pointers that are not aligned to their elements.
 * TC_ERR_WORKSPACE: a workspace that is null, too small or not 16-byte aligned.  Asynchronous on `stream`; nothing is
 * allocated after the graph's first calls on the device.  tc_debug_counter("den_accuracy_launches") and
 * ("den_accuracy_grad_launches") count the calls that launched their kernel. */
int64_t tc_den_expected_accuracy_workspace_bytes(const tc_den_graph *g, int32_t S, int32_t T);
int tc_den_expected_accuracy(tc_den_graph *g, int32_t S, const float *nnet_output, int64_t num_rows, int32_t num_cols,
                             int64_t row_stride, const int32_t *seq_frames_dev /* nullable: T each */, int32_t max_frames,
                             float leaky_hmm_coefficient, const int32_t *ref_dev /* [S * T] */,
                             const int32_t *class_dev /* nullable, [P] */, float *gamma, int64_t gamma_stride,
                             float *frame_acc_dev /* [S * T] */, double *acc_dev /* [S] */, void *workspace,
                             int64_t workspace_bytes, int device, void *stream);
int64_t tc_den_expected_accuracy_grad_workspace_bytes(const tc_den_graph *g, int32_t S, int32_t T);
int tc_den_expected_accuracy_grad(tc_den_graph *g, int32_t S, const float *nnet_output, int64_t num_rows, int32_t num_cols,
                                  int64_t row_stride, const int32_t *seq_frames_dev /* nullable: T each */,
                                  int32_t max_frames, float leaky_hmm_coefficient, const int32_t *ref_dev /* [S * T] */,
                                  const int32_t *class_dev /* nullable, [P] */, const float *frame_acc_dev /* [S * T] */,
                                  const float *seq_scale_dev /* nullable, [S]: 1 */, float *grad, int64_t grad_stride,
                                  void *workspace, int64_t workspace_bytes, int device, void *stream);

/* The same criterion against SOFT references: a dense per-pdf accuracy in place of ref_dev and class_dev,
 *     a_t(j) = accuracy[(t*S + s) * accuracy_stride + j],
 * held constant.  [K]'s chain-sMBR work (DenominatorSmbrComputation, `num_posteriors`) scores the denominator's paths against
 * the NUMERATOR'S posteriors this way, a_t(j) = gamma_num_t(j): a regular supervision allows several paths, and a hard
 * alignment of it under the current model moves with the model.  The matrix may hold any finite float32 -- posteriors,
 * label-smoothed indicators, signed rewards; nothing assumes [0, 1] -- and a power of two times the matrix gives that power
 * of two times every output, bit for bit (barring float32 underflow).  The float32 indicator of (ref_dev, class_dev) gives
 * the bits of tc_den_expected_accuracy / _grad.
 *   accuracy, accuracy_stride : device float32 (T*S, P), row t*S + s, rows accuracy_stride >= num_cols floats apart,
 *                 4-byte aligned.  Rows of padding frames are not read.
 * Every other argument, the outputs, the workspaces (tc_den_expected_accuracy_workspace_bytes,
 * tc_den_expected_accuracy_grad_workspace_bytes serve both pairs), the launches, the two forms of the gradient kernel and
 * "force_den_accuracy_streamed" are tc_den_expected_accuracy's and tc_den_expected_accuracy_grad's:
 *   frame_acc_dev : m_t = sum_j gamma_t(j) a_t(j): a lane's pdfs in order, double products and sums, then a butterfly over
 *                 the wave; rounded to float32.  acc_dev: their double sum in frame order.
 *   gamma       : on return the denominator posteriors -- which are also dE_s / da_t(j), the derivative in the matrix.
 *   The scan looks at the sequence's valid rows of `accuracy` as it looks at nnet_output's: a NaN or +-inf in either fails
 *   that sequence alone (acc NaN, NaN in its valid frames of frame_acc_dev, every gradient row +0); the other sequences
 *   keep their bits.
 *   The gradient kernel forms a_t(j) - m_t from the row where it reads nnet_output's row; everything behind that is the
 *   same code, with the error analysis of the hard form while |a - m| <= 1 (the error is relative to the scale of a).
 * TC_ERR_INVALID_ARGUMENT, before any device call: what the hard pair refuses, with `accuracy` null or not 4-byte aligned
 * and accuracy_stride < num_cols in place of the checks of ref_dev and class_dev.  TC_ERR_WORKSPACE, and TC_ERR_UNSUPPORTED
 * passed through for lengths on a graph of the streamed path, as there.  The launches count into "den_accuracy_launches" /
 * "den_accuracy_grad_launches" (and "..._grad_streamed_launches") and into "den_accuracy_dense_launches" /
 * "den_accuracy_dense_grad_launches". */
int tc_den_expected_accuracy_dense(tc_den_graph *g, int32_t S, const float *nnet_output, int64_t num_rows, int32_t num_cols,
                                   int64_t row_stride, const int32_t *seq_frames_dev /* nullable: T each */, int32_t max_frames,
                                   float leaky_hmm_coefficient, const float *accuracy /* (T*S, P) */, int64_t accuracy_stride,
                                   float *gamma, int64_t gamma_stride, float *frame_acc_dev /* [S * T] */,
                                   double *acc_dev /* [S] */, void *workspace, int64_t workspace_bytes, int device, void *stream);
int tc_den_expected_accuracy_dense_grad(tc_den_graph *g, int32_t S, const float *nnet_output, int64_t num_rows,
                                        int32_t num_cols, int64_t row_stride,
                                        const int32_t *seq_frames_dev /* nullable: T each */, int32_t max_frames,
                                        float leaky_hmm_coefficient, const float *accuracy /* (T*S, P) */,
                                        int64_t accuracy_stride, const float *frame_acc_dev /* [S * T] */,
                                        const float *seq_scale_dev /* nullable, [S]: 1 */, float *grad, int64_t grad_stride,
                                        void *workspace, int64_t workspace_bytes, int device, void *stream);

/* ---- paths drawn from the denominator's posterior (den_sample_kernels.hip) -----------------------------------------------
 * tc_den_sample_paths draws num_samples = K paths a sequence from P(path | y), the path posterior of the model that
 * tc_den_forward_backward sums over: p_t(j) = exp(clamp(y_t(j), +-30)), the graph's initial probabilities pi, every state
 * final, and the leaky-HMM transitions.  For any function r of a path, grad_y E[r] = E[(r - b) grad_y log P(path | y)] and
 * grad_y log P(path | y) = onehot(pdfs of the path) - gamma_den; with the risks centred over a sequence's K samples the gamma
 * term cancels and the estimate of the gradient is a scatter of K * T numbers: sequence-level risks (edit distance, any
 * reward) without a second forward-backward.  The random numbers are the caller's: `uniforms_dev`, float32 in [0, 1).
 *
 * The model.  With c the leaky coefficient, per sequence of T frames:
 *     alpha_0 = pi;   asum_t = sum_h alpha_t(h);   alpha'_t(h) = alpha_t(h) + c pi(h) asum_t
 *     alpha_{t+1}(g) = sum_{h->g} alpha'_t(h) w p_t(pdf) / asum_t
 * A latent path has levels t = 0 .. T.  At each level it holds the state it entered, pre_t, and the state it leaves from,
 * post_t; the two differ where a leak happened.
 * The selection rule.  For sequence s and sample k, u = uniforms[s][k] ((max_frames + 1) rows of 3):
 *     pick(weights, u) : the first index i, in list order, whose inclusive cumulative sum exceeds u * total.  Weights, sums
 *                        and the threshold are doubles.  If rounding leaves no such index, the last index with a positive
 *                        weight.  A zero weight is never picked.
 *     last state       : post_T = pick(alpha'_T over the states in state order, u[T][2]).
 *     for t = T down to 0, with j = post_t:
 *       leak decision  : no leak iff u[t][0] * alpha'_t(j) < alpha_t(j) (in double).  alpha'_t(j) is formed again from the
 *                        stored alpha_t(j), pi(j) and asum_t by the forward pass's own operations, so c = 0 never leaks.
 *       pre-leak state : pre_t = j without a leak, else pick(alpha_t over the states in state order, u[t][1]).
 *       arc, for t > 0 : the in-arcs of pre_t in the order of the graph's arc list, each weighted by the double product
 *                        alpha'_{t-1}(src) * w * p_{t-1}(pdf) (the frame's 1 / asum is common to the list and left out),
 *                        picked with u[t-1][2].  pdf_{t-1} is that arc's pdf and post_{t-1} its source.
 * Arithmetic.  alpha_t and asum_t are float32 where they are stored (the workspace); every sum over arcs or states is a
 * double sum rounded once when stored; p_t(j) is the float32 expf of the clamped output; w and pi are the handle's float32
 * probabilities; alpha'_t(h) = (float)((double)alpha_t(h) + (double)pi(h) * ((double)c * (double)asum_t)) wherever it is used;
 * alpha_{t+1}(g) = (float)(sum of the doubles alpha'_t(h) * (w * p_t(pdf)) times the double 1 / asum_t).  The double sums of
 * a pick may be associated in any way (chunks of 64 items, a prefix over the wavefront): that moves a threshold by about
 * 1e-16 of the total.
 * Failed sequences.  A sequence with a NaN or +-inf in its valid frames (the scan of tc_den_expected_accuracy_grad), or
 * with an asum_t that is zero, subnormal or not finite, or with sum_h alpha'_T(h) = 0, gets -1 in every slot; the other
 * sequences keep their bits.  Padding slots (frames >= the sequence's length, state levels above it) are -1.
 * A sequence's output depends only on its own rows of nnet_output, its own rows of uniforms_dev, the graph and c: not on S,
 * on its place in the batch, on K or on the other sequences.  Sample k of a K-sample call equals sample k of any other call
 * given the same uniforms[s][k].
 *   nnet_output : device float32 (T*S, P), row t*S + s, rows row_stride >= num_cols floats apart (2-D rows only, as the
 *                 expected-accuracy entries take); num_rows = S * max_frames.  Rows of padding frames are not read.
 *   seq_frames_dev : tc_den_best_path's: S device int32 lengths in 1 .. max_frames, or null (max_frames each).  Lengths work
 *                 on graphs of every size: this entry refuses no graph.
 *   uniforms_dev: device float32 [S][K][max_frames + 1][3], contiguous.  Row t of a sample: [0] the leak decision of level
 *                 t, [1] the pre-leak state of level t, [2] the arc of frame t (row T_s: the last state).
 *   pdf_dev     : device int32 [S][K][max_frames], 0-based pdfs.  state_dev (nullable): device int32
 *                 [S][K][max_frames + 1][2], (pre_t, post_t), the FST's states.
 *   workspace   : tc_den_sample_paths_workspace_bytes(g, S, max_frames): per sequence (T + 1) * Hs * 4 bytes (Hs: the
 *                 states rounded up to 4) plus T + 1 floats rounded up to 4; the whole rounded up to 256 bytes; 16-byte
 *                 aligned.
 * One launch, one workgroup a sequence; asynchronous on `stream`; the graph's training tables are not read (a training step
 * on the graph gives the same bits before and after) and nothing is allocated after the graph's first call on the device
 * (which uploads the tables of tc_den_expected_accuracy_grad if that has not).  The previous frame's alpha' is in LDS while
 * 4 * Hs + 1024 <= 163840 bytes, otherwise it is formed from the workspace's row per arc: the same bits
 * ("den_sample_streamed_launches" counts those launches, tc_debug_set("force_den_sample_streamed", 1) sends every graph
 * there).  "den_sample_launches" counts the launches; "den_launches" does not move.
 * TC_ERR_INVALID_ARGUMENT, before any device call: a null graph, nnet_output, uniforms_dev or pdf_dev; S, max_frames or
 * num_samples <= 0; num_rows != S * max_frames; num_cols != the graph's pdfs; row_stride < num_cols; a negative or
 * non-finite coefficient; a pointer that is not 4-byte aligned.  TC_ERR_WORKSPACE: a null, short or misaligned workspace. */
int64_t tc_den_sample_paths_workspace_bytes(const tc_den_graph *g, int32_t S, int32_t T);
int tc_den_sample_paths(tc_den_graph *g, int32_t S, const float *nnet_output, int64_t num_rows, int32_t num_cols,
                        int64_t row_stride, const int32_t *seq_frames_dev /* nullable */, int32_t max_frames,
                        float leaky_hmm_coefficient, int32_t num_samples, const float *uniforms_dev /* [S][K][T+1][3] */,
                        int32_t *pdf_dev /* [S][K][T] */, int32_t *state_dev /* nullable, [S][K][T+1][2]: pre, post */,
                        void *workspace, int64_t workspace_bytes, int device, void *stream);

/* ---- sampled paths scored on the device (path_edit_kernels.hip) ------------------------------------------------------------
 * tc_paths_edit_distance turns frame-level pdf paths -- what tc_den_sample_paths and tc_den_best_path write -- into token
 * sequences and scores each against its sequence's reference by the unit-cost Levenshtein distance: the risk of a
 * minimum-expected-edit-distance step and the errors of a free decoding, without a copy to the host.
 *
 * The tokens of a path.  pdf[s][k][t] is int32 [S][K][max_frames] (K = 1 for tc_den_best_path); sequence s has T_s =
 * seq_frames_dev[s] frames (clamped to 0 .. max_frames; null: max_frames each) and frames t >= T_s are never read.
 * token_of_pdf is int32 [P], pdf -> token id, a negative value meaning that the pdf emits nothing (silence);
 * start_of_pdf is uint8 [P] or null.  With c_t = token_of_pdf[pdf_t]:
 *   collapse mode (start_of_pdf null): frame t emits c_t iff c_t >= 0 && (t == 0 || c_t != c_{t-1}).  c_{t-1} is the frame
 *                  before's value whether or not that frame emitted: `a SIL a` gives `a a`, `a a` gives `a`.
 *   start mode   : frame t emits c_t iff c_t >= 0 && start_of_pdf[pdf_t] != 0 -- the chain topology's split into a forward
 *                  pdf and a self-loop pdf; it keeps `a a` apart.
 * The emitted values in frame order are the hypothesis h[0 .. N).  A path with a valid frame whose pdf lies outside
 * 0 .. P - 1 (the -1 of a failed sequence among them) is a failed path: len = -1, dist = -1 and -1 in every token slot.
 * The distance.  ref is int32 [S][max_ref], ref_len int32 [S] with M_s = ref_len[s] clamped to 0 .. max_ref; tokens compare
 * as plain integers; dist = the least number of insertions, deletions and substitutions that turn h[0 .. N) into
 * ref[s][0 .. M_s).  Integer arithmetic throughout: there is one answer.
 *   dist_dev, len_dev : device int32 [S][K]: the distance and N.
 *   tokens_dev  : nullable, device int32 [S][K][max_frames]: h, then -1.  When it is null the hypotheses lie in `workspace`
 *                 (tc_paths_edit_distance_workspace_bytes(S, K, max_frames) = 4 * S * K * max_frames rounded up to 256,
 *                 16-byte aligned), which is otherwise not looked at.
 *   max_ref     : 0 .. 4096.  With max_ref = 0, ref_dev and ref_len_dev may be null and dist = N: the tokens alone.
 * A path's outputs depend on its own row, its sequence's reference and the two maps alone: not on S, K or its place.
 * One launch, one wavefront a path, four independent wavefronts a workgroup; the previous row of the dynamic programme and
 * the reference lie in LDS (8 * max_ref rounded up to 64 bytes a wavefront).  Nothing is allocated, nothing is atomic; the
 * call is asynchronous on `stream` and may be captured.  "path_edit_launches" counts the launches.
 * TC_ERR_INVALID_ARGUMENT, before any device call: a null pdf_dev, token_of_pdf_dev, dist_dev or len_dev; ref_dev or
 * ref_len_dev null with max_ref > 0; S, K, max_frames or P <= 0; max_ref < 0; a pointer that is not 4-byte aligned.
 * TC_ERR_UNSUPPORTED, before any device call: max_ref > 4096; S * K >= 2^31.  TC_ERR_WORKSPACE: tokens_dev null and the
 * workspace null, short or misaligned. */
int64_t tc_paths_edit_distance_workspace_bytes(int32_t S, int32_t K, int32_t max_frames);
int tc_paths_edit_distance(int32_t S, int32_t K, const int32_t *pdf_dev /* [S][K][T] */,
                           const int32_t *seq_frames_dev /* nullable */, int32_t max_frames,
                           const int32_t *token_of_pdf_dev /* [P] */, const uint8_t *start_of_pdf_dev /* nullable, [P] */,
                           int32_t P, const int32_t *ref_dev /* [S][max_ref] */, const int32_t *ref_len_dev /* [S] */,
                           int32_t max_ref, int32_t *dist_dev /* [S][K] */, int32_t *len_dev /* [S][K] */,
                           int32_t *tokens_dev /* nullable, [S][K][T] */, void *workspace, int64_t workspace_bytes, int device,
                           void *stream);

/* tc_sampled_risk_grad: the gradient of sum_s grad_output[s] * L_s in the network output, L_s the surrogate of sampled
 * risks (functions.sampled_risk_surrogate):  L_s = sum_k weight[s][k] * sum_{t < T_s} clamp(y_s,t, +-30)[pdf[s][k][t]].
 * It clears the gradient (one memset of grad_elems elements) and launches one kernel.  For every (s, t < T_s) one thread
 * walks k = 0 .. K - 1; the first k to name a pdf owns the element (s, pdf, t) and stores, with one plain store,
 *     the double sum, in k order, of grad_output[s] * weight[s][k] (a double product) over the k whose sample has that
 *     pdf at t, rounded once to the element type (to nearest even, from the double),
 * provided that the pdf lies in 0 .. num_pdfs - 1 and -30 <= y <= 30 (inclusive, as clamp's backward; a NaN fails).  Every
 * other element is +0.  No atomics: the bits are a function of the inputs.
 *   pdf_dev [S][K][max_frames] int32; seq_frames_dev nullable [S] (clamped to 0 .. max_frames); weight_dev [S][K] and
 *   grad_output_dev [S] float64; input / grad: TC_DTYPE_* elements, element (s, c, t) at s * stride_s + c * stride_c +
 *   t * stride_t ((B, C, T) tensors by their strides; a 2-D (T*B, C) matrix has stride_s = its row stride and stride_t =
 *   B row strides).  grad is a block of grad_elems elements that holds every (s, c, t) at distinct places.
 * "sampled_risk_grad_launches" counts the launches.  TC_ERR_INVALID_ARGUMENT, before any device call: a null pdf_dev,
 * weight_dev, grad_output_dev, input or grad; S, K, max_frames or num_pdfs <= 0; an unknown dtype; a negative input
 * stride, a gradient stride <= 0 or a gradient element beyond grad_elems; a misaligned pointer.  TC_ERR_UNSUPPORTED:
 * K > 1024 (a thread compares its frame's K pdfs pairwise). */
int tc_sampled_risk_grad(int32_t S, int32_t K, int32_t max_frames, int32_t num_pdfs, const int32_t *pdf_dev,
                         const int32_t *seq_frames_dev /* nullable */, const double *weight_dev /* [S][K] */,
                         const double *grad_output_dev /* [S] */, const void *input, int dtype, int64_t input_stride_s,
                         int64_t input_stride_c, int64_t input_stride_t, void *grad, int64_t grad_stride_s,
                         int64_t grad_stride_c, int64_t grad_stride_t, int64_t grad_elems, int device, void *stream);

/* ---- the denominator graph's weights on caller-built supervisions ------------------------------------------------------
 * Every supervision Kaldi writes into an eg has been composed with the normalization FST of den.fst ([K]
 * AddWeightToSupervisionFst, DenominatorGraph::GetNormalizationFst; the end-to-end egs: --normalization-fst-scale), which
 * makes the numerator a weighted subset of the denominator's paths -- a path the phone LM forbids is gone, one it allows
 * carries -log pi(h_0) - sum log w -- and so bounds the objective by 0.  (The reference takes such supervisions from the
 * egs: src/my_lib.h:21.)  tc_den_compose does that for supervisions the caller built.  Host code only: no GPU is
 * touched, the graph is only read (tc_den_graph_hash and every result of a step on it stay what they were), and any number
 * of threads may call it on one handle.
 *
 * The normalization acceptor N of a graph: the states of den.fst plus a start q0; every arc h -> h' (pdf p, probability w)
 * at cost -log w; for every state h with pi(h) > 0 and every arc h -> h' an arc q0 -> h' with label p at cost
 * -log pi(h) - log w (the epsilon-removed form); every state final at cost 0.  pi and w are the handle's float32 values
 * (tc_den_graph_initial_probs, tc_den_graph_arcs: the ones the denominator kernels use), the logarithms are float64; an
 * arc with w == 0 is on no path and is left out.  N's costs are multiplied by `scale` (finite, >= 0; [K] e2e
 * normalization_fst_scale; 0 only restricts the paths).  The leaky-HMM coefficient does not enter.
 *
 * Input: S acceptors concatenated exactly as tc_supervision_create_ragged (e2e == 0: `start` is not read, state 0 starts
 * every sequence) or tc_supervision_create_e2e (e2e != 0) take them.  Output, per sequence, the product with N: start
 * (s_0, q0); an arc (s, h) --p--> (s', h') for every pair of an input arc and an arc of N with its label, at cost
 * float32(double(c_sup) + scale * c_N); the final cost of (s, h) is that of s; trimmed to the states that are reachable and
 * lead to a final state.  Two arcs of N with the same source and label stay two arcs: nothing is determinised or
 * minimised, so a non-deterministic den.fst is summed over.  ([K] determinises in the tropical semiring afterwards, which
 * would keep only the best of the start states' terms; here several LM histories per supervision state stay alive for
 * the first few phones, which costs states and keeps the sum.)
 * Order (the same input gives the same bytes): breadth-first from the start, states taken in increasing new id, their
 * input arcs in input order, for each the matching arcs of N in the order the handle keeps the graph's arcs (for q0:
 * h ascending, then its arcs); a state gets the next id when first reached; trimming keeps the relative order.  The start
 * is state 0 of every output, and a time-unfolded input comes out in time order: what tc_supervision_create_ragged asks.
 * Status per sequence: 0; 1 = the product is empty (no path of the input is in the graph); 2 = the product has more than
 * max_states states before trimming ([K] kSupervisionMaxStates = 200000) or does not fit the int32 offsets.  A sequence of
 * status 1 or 2 has no states in the output and changes nothing for the others: every sequence's output is that of the
 * call on it alone.
 * Size: composed end-to-end acceptors can exceed TC_E2E_MAX_STATES / TC_E2E_MAX_ARCS (tc_supervision_create_e2e_any takes them), composed regular ones can move
 * from the resident to the level-windowed numerator; tc_den_compose_info and tc_supervision_stats tell beforehand.
 * TC_ERR_BAD_FST (nothing is read out of bounds): offsets that do not start at 0 or decrease, a sequence without states,
 * a label outside 1 .. label_dim, a next state or start outside the sequence, a NaN or -inf cost.  A label above the
 * graph's number of pdfs matches nothing.  TC_ERR_INVALID_ARGUMENT: a null pointer, S, label_dim or max_states < 1, a
 * scale that is negative or not finite.
 * The result is owned by the caller (tc_den_compose_free).  tc_den_compose_sizes: out3 = {S, states, arcs} of the
 * concatenated output.  tc_den_compose_info: status[S] and info4[S][4] = states, arcs of the input and of the output (any
 * pointer may be NULL).  tc_den_compose_copy: the output's arrays in the layout of the input (seq_state_begin S + 1, start
 * S, arc_begin states + 1, ...; any pointer may be NULL).
 * tc_den_graph_arcs: the graph's arcs as the handle keeps them (num_arcs entries each, host memory, any may be NULL):
 * source, destination, 0-based pdf, probability. */
typedef struct tc_den_compose_result tc_den_compose_result;
int tc_den_graph_arcs(const tc_den_graph *graph, int32_t *src, int32_t *dst, int32_t *pdf, float *prob);
int tc_den_compose(tc_den_compose_result **out, const tc_den_graph *graph, int32_t num_sequences, int32_t label_dim,
                   int e2e, const int32_t *seq_state_begin, const int32_t *start /* e2e only */, const int32_t *arc_begin,
                   const int32_t *arc_ilabel, const float *arc_weight, const int32_t *arc_nextstate,
                   const float *final_weight, float scale, int64_t max_states);
int tc_den_compose_sizes(const tc_den_compose_result *result, int64_t *out3);
int tc_den_compose_info(const tc_den_compose_result *result, int32_t *status, int64_t *info4);
int tc_den_compose_copy(const tc_den_compose_result *result, int32_t *seq_state_begin, int32_t *start, int32_t *arc_begin,
                        int32_t *arc_ilabel, float *arc_weight, int32_t *arc_nextstate, float *final_weight);
void tc_den_compose_free(tc_den_compose_result *result);

/* The cross-entropy objective Kaldi's chain trainer reports next to the chain objective ([K]
 * nnet-chain-training.cc: TraceMatMat(xent_output, xent_deriv, kTrans), xent_deriv = w * numerator posteriors);
 * the reference leaves it as a TODO (torchain/functions.py:88-89).  objf_dev: device double[1].  Needs
 * tc_chain_workspace_bytes-sized or at least 4096 bytes of 16-byte aligned device scratch. */
int tc_xent_objf(const float *xent_output, int64_t num_rows, int32_t num_cols, int64_t output_stride,
                 const float *xent_output_deriv, int64_t deriv_stride, double *objf_dev, void *workspace,
                 int64_t workspace_bytes, int device, void *stream);

/* Diagnostics for bench.py / DESIGN.md: copies a few schedule statistics of the graph
 * (out[0]=padded forward arc slots, out[1]=padded backward arc slots, out[2]=LDS bytes of the fused
 * kernel for this graph, out[3]=threads per workgroup, out[4]=forward rows, out[5]=backward rows,
 * out[6], out[7] = forward / backward LDS bank-conflict factor of the placed arc gathers x 1000, where
 * 1000 means conflict-free; out[8] = 1 when the graph is "tied" -- all non-self-loop arcs entering a
 * state carry one pdf, possibly after state splitting -- and runs a factorised on-chip kernel (one-stream forms up to
 * 16384 layout positions, the plane-wise form up to 28672, with its gather source in LDS a half at a time up to 40960), 2 when
 * the graph is too large for the on-chip layouts and runs the streamed kernel, 0 for a general on-chip kernel (up to 8192 states: on
 * owner-computes schedules). */
int tc_den_graph_stats(const tc_den_graph *graph, int64_t *out9);

/* Kernel choice of batches above one sequence per two CUs.  Tied on-chip graphs of up to 8192 positions have two
 * kernels: the fused one (one sequence per workgroup) and the two-sequence one (a pair of sequences on two CUs that
 * share the arc walk), which is the faster from about 11 arcs per state on.  tc_den_graph_prepare times both once per
 * graph and device on a zero-filled scratch batch (one sequence per CU, 48 frames; the scratch, about
 * 2 * CUs * 48 * num_pdfs * 4 bytes plus that batch's workspace, is freed again) and keeps the two-sequence kernel
 * when it is at least 3% faster; tc_debug_set("no_tune", 1) or ("no_pair", 1) before the graph's first use on the
 * device keeps the fused kernel, ("force_pair", 1) selects the other wherever it fits.  Both kernels agree with the
 * reference to the same tolerance; their results differ from each other in the last bits.
 * Reports the choice (1 = two-sequence kernel) and the two times in ms; prepares the graph if it was not. */
int tc_den_graph_tuning(tc_den_graph *graph, int device, int32_t *two_sequence_kernel, float *fused_ms,
                        float *two_sequence_ms);

/* Fixes that choice instead of timing it: two_sequence_kernel = 0 / 1, or -1 to forget a fixed choice (the next
 * tc_den_graph_prepare on the device times again).  Called BEFORE the graph first reaches `device` no timing launch is
 * made at all; called later the choice applies from the next launch on.  This is what makes the choice reproducible:
 * each kernel is bitwise reproducible by itself, the two differ in the last bits, and a timing race decides by clock
 * noise for a graph near the 3 % threshold -- from run to run and from rank to rank.  Since round 5 the LIBRARY keeps the
 * cache of measured choices (csrc/tuning_cache.cpp): tc_den_graph_prepare looks the graph up -- key: tc_den_graph_hash +
 * the device's name -- in the JSON file $TORCHAIN_TUNING_CACHE (else ~/.cache/torchain_amd/tuning.json) before it times
 * anything and stores what it timed, so a caller of this ABI gets the same kernel run after run without calling this
 * function; the Python wrapper applies rank 0's choice on every rank of a data-parallel job
 * (parallel.sync_den_graph_variant).
 * (The reference's call is deterministic for fixed inputs: src/my_lib_chain.cpp:129-131.) */
int tc_den_graph_set_variant(tc_den_graph *graph, int device, int32_t two_sequence_kernel);
/* 64-bit FNV-1a hash of the graph (sizes, arcs, pdfs, probabilities): the key of such a cache.  0 for a null handle. */
uint64_t tc_den_graph_hash(const tc_den_graph *graph);
/* That cache, directly (host only; e.g. to ship the choices measured on one machine to a fleet): 1 / 0 = found / not. */
int tc_tuning_cache_get(uint64_t graph_hash, const char *device_name, int32_t *two_sequence_kernel);
int tc_tuning_cache_put(uint64_t graph_hash, const char *device_name, int32_t two_sequence_kernel, float fused_ms,
                        float two_sequence_ms);

/* ---- layout conversion either side of the path -------------------------- */

/* Replaces `to2d` (torchain/functions.py:118-125: x.permute(2,0,1).contiguous().view(-1, C)):
 * in_bct is a contiguous (B, C, T) device tensor, out2d[(t*B + b) * out_stride + c] = in_bct[b][c][t]. */
int tc_to2d(const float *in_bct, int32_t B, int32_t C, int32_t T, float *out2d, int64_t out_stride, int device,
            void *stream);

/* The way back, fused with the sign / scale the reference applies in separate passes
 * (torchain/functions.py:108-112: -mmi_grad, -xent_regularize * xent_grad, then autograd's inverse permute):
 * out_bct[b][c][t] = scale * in2d[(t*B + b) * in_stride + c],  out_bct contiguous (B, C, T). */
int tc_from2d(const float *in2d, int64_t in_stride, int32_t B, int32_t C, int32_t T, float scale, float *out_bct,
              int device, void *stream);

/* The counterparts of tc_to2d / tc_from2d for a channel-last view (TC_LAYOUT_CHANNEL_LAST of tc_chain_step_strided; the
 * permutation of torchain/functions.py:118-125 with the channels already last), on tensors of `dtype` (TC_DTYPE_*):
 *   out2d[(t*B + b) * out_stride + c] = (float) in[b*batch_stride + t*frame_stride + c]        (an exact widening)
 * Strides in elements, checked as tc_chain_step_strided checks them.  One wave per row; 16-byte accesses when C, both
 * strides (4 elements for float32, 8 for 16-bit tensors), out_stride and both base addresses allow them, else element-wise. */
int tc_rows_gather(const void *in, int dtype, int32_t B, int32_t C, int32_t T, int64_t batch_stride, int64_t frame_stride,
                   float *out2d, int64_t out_stride, int device, void *stream);

/* The way back into a DENSE (B, T, C) tensor of `dtype`, with what tc_chain_step_strided applies to the MMI gradient:
 *   out_btc[(b*T + t)*C + c] = round(f(in2d[(t*B + b) * in_stride + c]))
 *   f(v) = scale * v                                  row_weights == NULL, out_of_range_regularize == 0
 *        = (scale * w[t*B + b]) * v                   row_weights given: one float32 multiply of v
 *        = w[t*B + b] * (scale * v + fl32(2c) * p(y)) out_of_range_regularize = c > 0 (w = 1 without row_weights): the penalty
 *          of tc_chain_step_penalized with y = input[b*batch_stride + t*frame_stride + c]; an element with p(y) == 0 keeps
 *          the bits of scale * v (times w)
 * rounded once to nearest even for 16-bit tensors.  input, batch_stride and frame_stride are read only with c > 0. */
int tc_rows_scatter(const float *in2d, int64_t in_stride, int dtype, int32_t B, int32_t C, int32_t T, float scale,
                    const float *row_weights, float out_of_range_regularize, const void *input, int64_t batch_stride,
                    int64_t frame_stride, void *out_btc, int device, void *stream);

/* Diagnostic, host only: replays one arc walk from the graph's built schedules exactly as the kernels
 * consume them and returns, per state, direction 0: sum over in-arcs (h->g) of w*gather[h]*pdf_factor[pdf],
 * direction 1: sum over out-arcs (h->g) of w*gather[g]*pdf_factor[pdf]  (gather: num_states floats,
 * pdf_factor: num_pdfs floats, out: num_states floats).  Lets the schedule builder be tested without a GPU;
 * nothing on the hot path calls it. */
/* Diagnostic, host only: process-wide switches; they exist so that tests and profiles can put a graph or a batch on
 * a kernel family it would not normally take.  Read when a graph is BUILT (tc_den_graph_create / _read):
 *   "force_general"  (1: never use the tied-graph kernel)      "force_streamed" (1: alpha/beta in HBM, as for graphs
 *   "no_split"       (1: do not tied-ify nearly tied graphs)                     beyond the on-chip layouts)
 *   "no_pdf_banks", "no_pdf_search", "no_bank_search" (1: skip those placement passes)   "phantom_pdf0" (1: unused positions of a tied layout on pdf 0, as before round 5)
 *     "sched_trace" (1: builder statistics on stderr)
 *   "slab_wide" / "slab_narrow" (1: the streamed path cuts the batch into slabs of 32 / 16 sequences whatever the graph's size)
 *   "old_arrange"    (1: the greedy placement of a half-slot's cells that rounds 1-4 used, instead of round 5's matching:
 *                     HISTORY.md 4.1e)
 *   "no_planes"      (1: tied graphs of 16385..40960 positions take the streamed path, not the plane-wise on-chip kernel)
 *   "no_split_source" (1: tied graphs of 28673..40960 positions take the streamed path at every batch, as before round 6)
 *   "old_general"    (1: general graphs take round 1's on-chip kernel, not the one on owner-computes schedules)
 * Read at launch (one relaxed atomic load):
 *   "no_phase_split" (1: batches of at most 128 sequences of tied on-chip graphs take the fused kernel instead of
 *                     running forward and backward recursion on two CUs at once; the plane-wise kernel likewise)
 *   "no_num_overlap" (1: the numerator always follows the denominator on the caller's stream; by default it runs
 *                     beside it on a side stream when the denominator leaves CUs idle)
 *   "force_pair"     (1: the two-sequence kernel wherever it fits, whatever the batch and the graph's timing said)
 *   "no_mitm" / "force_mitm" (two CUs per sequence: never / always the form that meets in the middle instead of
 *                     two pure recursions and a combining pass; by default from 32 / 48 / 64 sequences by layout class)
 *   "planes_meet_at" (M > 0: the two-workgroup form of the plane-wise kernel meets at frame M instead of T / 2 -- measured:
 *                     T / 2 is the balanced choice, profiles/r06_planes_ab.txt)
 *   "exp_per_frame"  (1: the streamed path transposes exp(y) one frame at a time, as it does when all frames would take
 *                     more than 1 GB of workspace)
 *   "force_num_windowed" (1: regular supervisions that fit the resident numerator kernel take the level-windowed one,
 *                     which otherwise serves those that do not fit; same bits.  Read at every numerator launch and by
 *                     tc_supervision_stats)
 *   "force_den_best_path_streamed" (1: tc_den_best_path reads the previous frame's scores from the workspace for every
 *                     graph, as it does for those beyond its LDS form; same bits.  Read at every such call)
 *   "force_num_e2e_large" (1: end-to-end supervisions that fit the resident numerator kernel take num_e2e_large_kernels.hip,
 *                     which otherwise serves those that do not fit; same bits.  Read when a supervision first reaches a device
 *                     -- its pool slot then gets the 4 bytes per arc that kernel needs -- at every numerator launch and by
 *                     tc_supervision_e2e_stats; a launch on a handle staged before the switch was set returns
 *                     TC_ERR_UNSUPPORTED before anything is enqueued or counted)
 *   "no_full_layout" (1: the fused tied kernel never runs its full-layout twin -- every plane of states and pdfs whole,
 *                     16-byte rows, no cross-entropy zero rows, no hub states, DESIGN.md 4.1 -- but the general
 *                     instantiation; same bits.  Read at every such launch)
 *   "force_den_accuracy_streamed" (1: tc_den_expected_accuracy_grad and tc_den_expected_accuracy_dense_grad keep their
 *                     per-frame vectors in the workspace for every graph, as they do for those beyond the LDS form; same
 *                     bits.  Read at every such call)
 *   "force_den_sample_streamed" (1: tc_den_sample_paths forms the previous frame's alpha' from the workspace's row for
 *                     every graph, as it does for those beyond the LDS form; same bits.  Read at every such call)
 * Read when a graph first reaches a device (tc_den_graph_prepare, see tc_den_graph_tuning):
 *   "no_pair"        (1: never the two-sequence kernel)        "no_tune" (1: no timing launches; the fused kernel)
 * The same switches can be set from the environment when the library is loaded:
 *   TORCHAIN_HIP_DEBUG="no_tune,force_streamed=1"   (unknown keys are reported on stderr and ignored).
 * Returns TC_ERR_INVALID_ARGUMENT for an unknown key. */
int tc_debug_set(const char *key, int value);
/* Diagnostic counters: "pool_device_allocs" = device allocations made so far by the per-device supervision pool
 * (stops growing once the pool is warm: a training step then allocates and frees nothing), "pool_reuses" = slots
 * handed out again; "den_launches" / "den_backward_launches" / "num_launches" / "num_backward_launches" /
 * "layout_launches" = denominator computations enqueued / those with a backward recursion / numerator computations /
 * those with a backward recursion / (B, C, T) <-> (T*B, C) copies, process-wide since the library was loaded;
 * (tc_den_graph_prepare's one-off timing launches of a graph's two kernels are counted like any other);
 * "den_long_utterance_launches" = on-chip denominator launches whose frame sums did not fit LDS and went through the
 * workspace (utterances of many hundred frames on the largest on-chip graphs); "num_e2e_staged_launches" = end-to-end
 * numerator launches that ran beside the denominator and left their posteriors for the scatter kernel;
 * "num_windowed_launches" = regular numerator launches that took the level-windowed kernel (counted in "num_launches" too);
 * "channel_last_steps" = tc_chain_step_strided calls taken in TC_LAYOUT_CHANNEL_LAST (their row gathers and scatters, and
 * tc_rows_gather / tc_rows_scatter, count as "layout_launches"); "ragged_steps" = objective calls made on a ragged
 * supervision (tc_supervision_create_e2e_ragged, tc_supervision_create_ragged; their padding kernels are not counted as
 * "layout_launches");
 * "ragged_two_cu_launches" = denominator launches of a ragged batch that took two workgroups per sequence, each sequence
 * meeting at half its own length (tied graphs, 8 sequences up to half the device's CUs, a derivative asked for, neither
 * "no_mitm" nor "no_phase_split" set; counted in "den_launches" too);
 * "best_path_launches" = tc_supervision_best_path calls that launched their kernel (not counted in "num_launches");
 * "den_best_path_launches" = tc_den_best_path calls that launched their kernel (not counted in "den_launches"), and
 * "den_best_path_streamed_launches" those of them that read the previous frame's scores from the workspace;
 * "xent_log_softmax_launches" = launches of tc_chain_step_log_softmax's two kernels (the row statistics and the gradient
 * pass: 2 a training step, 1 an evaluation step that asks for xent_objf_dev, 0 with the switch off);
 * "num_e2e_large_launches" = end-to-end numerator launches that took num_e2e_large_kernels.hip (counted in "num_launches" too);
 * "tied_full_layout_launches" = launches of the fused tied kernel's full-layout twin (counted in "den_launches" too);
 * "den_accuracy_launches" = tc_den_expected_accuracy calls that launched their row kernel (the denominator launch in front of
 * it counts in "den_launches" and "den_backward_launches" as any other), "den_accuracy_grad_launches" =
 * tc_den_expected_accuracy_grad calls that launched their kernel, and "den_accuracy_grad_streamed_launches" those of them
 * that kept the per-frame vectors in the workspace; "den_accuracy_dense_launches" and "den_accuracy_dense_grad_launches" =
 * those of the first two that came through tc_den_expected_accuracy_dense and tc_den_expected_accuracy_dense_grad;
 * "den_sample_launches" = tc_den_sample_paths calls that launched their kernel (not counted in "den_launches"), and
 * "den_sample_streamed_launches" those of them that formed the previous frame's alpha' from the workspace;
 * "path_edit_launches" = tc_paths_edit_distance calls that launched their kernel, "sampled_risk_grad_launches" = those of
 * tc_sampled_risk_grad;
 * "boost_launches" = launches of boost_kernels.hip: 1 a tc_boost_rows call; 1 a tc_chain_step_boosted call with
 * l2_regularize == 0, 3 a training step and 2 an evaluation step with it (the pass, the sequences' sums, the gradient's
 * fix-up); 0 for every other entry.
 * -1 for an unknown key. */
int64_t tc_debug_counter(const char *key);

int tc_den_graph_debug_walk(const tc_den_graph *graph, int direction, const float *gather,
                            const float *pdf_factor, float *out);

#ifdef __cplusplus
}
#endif
#endif /* TORCHAIN_HIP_H_ */
