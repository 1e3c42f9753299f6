/*
 * lddl_amd — C ABI of the MI355X-native BERT preprocessing hot path.
 *
 * The reference (wdykas/LDDL) is pure Python; its hot path calls into the HF `tokenizers` Rust
 * extension, `random`, numpy and CPU torch from Python. Each entry point below replaces one of
 * those call sites and is bound from Python with ctypes (INTEGRATION.md shows the stubs).
 *
 * Conventions
 *   - Plain C types only. `d_*` arguments are DEVICE pointers (HBM, e.g. torch.cuda tensors'
 *     data_ptr()), `h_*` arguments are host pointers. `stream` is a hipStream_t passed as void*
 *     (NULL = the legacy default stream). All device work is asynchronous on `stream`
 *     unless the function says otherwise.
 *   - Return value: 0 on success, negative on error; lddl_last_error() returns a thread-local
 *     message for the last failing call.
 *   - One lddl_ctx per device; a ctx may be shared by host threads only with external locking.
 *     Never create a ctx before fork() in a process whose children touch the GPU.
 */
#ifndef LDDL_AMD_H_
#define LDDL_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lddl_ctx lddl_ctx;

/* ---------------------------------------------------------------------------------------------
 * Errors / version
 * ------------------------------------------------------------------------------------------- */
const char* lddl_last_error(void);
int lddl_version(void);
/* Build identity: the first 16 hex digits of a SHA-256 over this library's sources (csrc/ and
 * include/, as compiled), so that a measurement (bench line, PMC pass) can name the exact build
 * it ran; no reference counterpart. */
const char* lddl_build_id(void);

/* ---------------------------------------------------------------------------------------------
 * Synthetic corpus; host-only, no GPU needed.
 * Generates documents [doc_begin, ...) of the deterministic corpus until >= target_bytes of
 * sentence text. Output: concatenated sentence bytes, sent_off[n_sent+1] (byte offsets),
 * doc_sent_off[n_doc+1] (sentence offsets). Returns the number of text bytes (<0 on overflow).
 * ------------------------------------------------------------------------------------------- */
int64_t lddl_synth_corpus(uint64_t seed, int64_t doc_begin, int64_t target_bytes,
                          double nonascii_frac, uint8_t* text, int64_t text_cap,
                          int64_t* sent_off, int64_t sent_cap, int64_t* doc_sent_off,
                          int64_t doc_cap, int64_t* n_sent_out, int64_t* n_doc_out,
                          int n_threads);
/* The same synthetic documents as raw document text (sentences joined by one space), for the
 * segmentation path: text[doc_off[d] .. doc_off[d+1]). Returns the byte count (< 0: capacity). */
int64_t lddl_synth_doc_text(uint64_t seed, int64_t doc_begin, int64_t target_bytes,
                            double nonascii_frac, uint8_t* text, int64_t text_cap, int64_t* doc_off,
                            int64_t doc_cap, int64_t* n_doc_out, int n_threads);

/* ---------------------------------------------------------------------------------------------
 * Host reader of the preprocessor input (host-only, no GPU): replaces the per-line Python of
 * dask.bag.read_text + random_sample (lddl/dask/readers.py:60-71), split_id_text (readers.py
 * :131-136) and the document shuffle (lddl/dask/bert/pretrain.py:100-111, here per shuffle group
 * with CPython's Random(seed).shuffle) for a batch of blocks, in threads.
 * lddl_read_groups: block i = bytes [starts[i], ends[i]) of file paths[i]; mt_states (may be NULL:
 *   no sampling) holds 625 words per block (the 624-word random_sample state + its index); a line
 *   (block split on '\n', str.strip()ed, empty dropped) is kept iff random() < ratio. Blocks are
 *   grouped into shuffle groups by group_off[n_groups+1]; group g's documents are shuffled by
 *   random.Random(s).shuffle with abs(s) = group_seed_abs[g] and dealt back over its blocks (each
 *   keeps its count). Every block must be valid UTF-8 (dask decodes blocks strictly): else
 *   returns -2 with bad[0] = block, bad[1] = byte offset in the block. On success *n_docs
 *   documents of *n_text bytes (the text after each line's id) are held by *out.
 * lddl_read_fill: text[n_text], doc_off[n_docs+1], block_ndocs[n_blocks] (may be NULL), in block
 *   order. lddl_read_free releases the handle.
 * ------------------------------------------------------------------------------------------- */
typedef struct lddl_reader lddl_reader;
int lddl_read_groups(int64_t n_blocks, const char* const* paths, const int64_t* starts,
                     const int64_t* ends, const uint32_t* mt_states, double ratio, int64_t n_groups,
                     const int64_t* group_off, const uint64_t* group_seed_abs, int n_threads,
                     lddl_reader** out, int64_t* n_docs, int64_t* n_text, int64_t* bad);
int lddl_read_fill(lddl_reader* reader, uint8_t* text, int64_t* doc_off, int64_t* block_ndocs);
/* block_ndocs[n_blocks] and doc_len[n_docs] (text bytes per document), either may be NULL; then
 * lddl_read_fill_range copies documents [d0, d1) only: text[sum of their lengths],
 * doc_off[d1 - d0 + 1] relative to text (a GPU batch at a time). */
int lddl_read_counts(const lddl_reader* reader, int64_t* block_ndocs, int64_t* doc_len);
int lddl_read_fill_range(lddl_reader* reader, int64_t d0, int64_t d1, uint8_t* text,
                         int64_t* doc_off);
int lddl_read_free(lddl_reader* reader);
/* dask 2021.10 `random_state_data_python(n, seed)` (the per-partition MT states of
 * bag.random_sample): n states of 624 words = Random(abs(seed)).randint(0, 2**32) in order, each
 * followed by the index 624 (as setstate stores them: 2**32 becomes 0). out[625 * n]. */
int lddl_random_state_data(int64_t n, uint64_t seed_abs, uint32_t* out);

/* ---------------------------------------------------------------------------------------------
 * Context = device-resident tokenizer tables.
 * Replaces `transformers.BertTokenizerFast(vocab_file)` (lddl/dask/bert/pretrain.py:584-587,
 * lddl/torch/bert.py:343-346). `norm_table` is lddl_amd/assets/bert_norm_{uncased,cased}.bin
 * (lowercase=True is the reference default); `vocab` is the raw vocab.txt bytes,
 * token id = line number. special_ids order: [PAD] [UNK] [CLS] [SEP] [MASK] (-1 if absent).
 * ------------------------------------------------------------------------------------------- */
int lddl_ctx_create(int device, const uint8_t* norm_table, int64_t table_len, const char* vocab,
                    int64_t vocab_len, lddl_ctx** out);
int lddl_ctx_destroy(lddl_ctx* ctx);
int lddl_ctx_info(const lddl_ctx* ctx, int32_t* vocab_size, int32_t* special_ids,
                  int32_t* max_piece_bytes);
/* Bytes per token id in the pair tables (lddl_pairs_emit tokens and labels, the render inputs):
 * 2 (uint16) when vocab_size <= 65534 (two 16-bit values stay free for the gather's decision
 * table), else 4 (int32). */
int lddl_ctx_id_bytes(const lddl_ctx* ctx);
/* device pointers to the vocab strings (for rendering ' '.join(tokens)): token i is
 * bytes[off[i] .. off[i+1]) */
int lddl_ctx_render_table(const lddl_ctx* ctx, const uint8_t** d_bytes, const int64_t** d_off);

/* Device allocator of the library's per-call temporaries (pair plans, scans, binning scratch).
 * Default: the ctx's own cache of hipMalloc blocks. With callbacks set, every temporary comes
 * from alloc_fn(bytes, stream, user) and goes back through free_fn(p, stream, user) on the
 * stream of its last use — a stream-ordered pool such as PyTorch's caching allocator
 * (lddl_amd/context.py), so one allocator owns HBM. Both NULL restores the default. */
typedef void* (*lddl_alloc_fn)(size_t bytes, void* stream, void* user);
typedef void (*lddl_free_fn)(void* p, void* stream, void* user);
int lddl_ctx_set_allocator(lddl_ctx* ctx, lddl_alloc_fn alloc_fn, lddl_free_fn free_fn,
                           void* user);

/* ---------------------------------------------------------------------------------------------
 * Tokenize sentences (device in, device out).
 * Replaces `tokenizer.tokenize(s, max_length=512, truncation=True)` per Punkt sentence
 * (lddl/dask/bert/pretrain.py:79-80, 89-92).
 *   d_text[n_bytes], d_sent_off[n_sent+1] (int64 byte offsets; sentence s = text[off[s]:off[s+1]])
 *   -> d_ids[n_bytes] (int32): sentence s's pieces at d_ids[off[s] ...] (pieces <= bytes)
 *   -> d_sent_len[n_sent] (int32): kept piece count (<= max_pieces) | 1<<30 if they contain a
 *      literal [CLS]/[SEP]. A count of 0 means the sentence is dropped (pretrain.py:92).
 * ------------------------------------------------------------------------------------------- */
int lddl_tokenize(lddl_ctx* ctx, void* stream, const uint8_t* d_text, int64_t n_bytes,
                  const int64_t* d_sent_off, int64_t n_sent, int32_t max_pieces, int32_t* d_ids,
                  int32_t* d_sent_len);

/* ---------------------------------------------------------------------------------------------
 * UTF-8 validation (the strict decode dask.bag.read_text applies to every input block, readers.py
 * :60-71; the reference raises UnicodeDecodeError on malformed input): *d_first_bad (device int64)
 * = offset of the first byte that does not begin or continue a well-formed sequence (Python's
 * decoder rules: no overlongs, surrogates or > U+10FFFF), or 0x7F7F7F7F7F7F7F7F if all of
 * d_text[0 .. n_bytes) is valid. Asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------- */
int lddl_utf8_check(void* stream, const uint8_t* d_text, int64_t n_bytes, int64_t* d_first_bad);

/* ---------------------------------------------------------------------------------------------
 * Punkt sentence segmentation (device in, device out).
 * Replaces `nltk.tokenize.sent_tokenize(text)` + `strip()` + dropping empty sentences
 * (lddl/dask/bert/pretrain.py:86-88) for every document of a batch: nltk 3.6.5's
 * PunktSentenceTokenizer(params).span_tokenize (nltk/tokenize/punkt.py:1316-1391, realign
 * 1351-1379, annotation 582-630 / 1516-1650): kernels in segment.hip, annotation in punkt_dev.h,
 * the tables of lddl_punkt_set_params in punkt.hip (parsed on the host by punkt_params.h).
 * lddl_punkt_set_params: `table` = lddl_amd/assets/punkt_props.bin (Python's character classes),
 *   `records` = the PunktParameters (abbrev_types, sent_starters, ortho_context, collocations)
 *   as records (u8 kind 1/2/3/4, u8 value = ortho flags, u16 len_a, u16 len_b, UTF-8 bytes a, b);
 *   records_bytes = 0 is the untrained PunktSentenceTokenizer(). Keys longer than 255 bytes are
 *   rejected. Must be called once before lddl_segment_count.
 * lddl_segment_count: documents d_text[d_doc_off[d] .. d_doc_off[d+1]) (the text after the
 *   document id, readers.py:131-136; documents contiguous, each < 2 GiB, valid UTF-8, inside
 *   [0, n_bytes)); returns the sentence count
 *   (synchronises the stream). Exactly one lddl_segment_fill must follow on the same ctx.
 * lddl_segment_fill -> d_sent_off[n_sent+1], d_doc_sent_off[n_doc+1]: sentence k of document d
 *   is d_text[sent_off[doc_sent_off[d]+k] .. sent_off[...+1]); it equals the reference's
 *   stripped sentence up to leading/trailing whitespace (sentences are contiguous: whitespace
 *   between sentences is attached to the left one, which the BERT tokenizer ignores), and a
 *   whitespace-only sentence stands for the reference's dropped empty string (0 pieces, dropped
 *   by the pair builder exactly like pretrain.py:92-97). The output feeds lddl_tokenize.
 *   Both outputs NULL cancels the pending segmentation (releases its scratch; the host calls it
 *   when something fails between count and fill).
 * ------------------------------------------------------------------------------------------- */
int lddl_punkt_set_params(lddl_ctx* ctx, const uint8_t* table, int64_t table_bytes,
                          const uint8_t* records, int64_t records_bytes);
int lddl_segment_count(lddl_ctx* ctx, void* stream, const uint8_t* d_text, int64_t n_bytes,
                       const int64_t* d_doc_off, int64_t n_doc, int64_t* n_sent);
int lddl_segment_fill(lddl_ctx* ctx, void* stream, int64_t* d_sent_off, int64_t* d_doc_sent_off);

/* ---------------------------------------------------------------------------------------------
 * BART pretraining chunks (device in, device out).
 * Replaces `_aggregate_sentences` (lddl/dask/bart/pretrain.py:88-128) for every document of a
 * batch, over the layout lddl_segment_fill writes: per document, in sentence order,
 *   chunk += " " + sentence.strip(); num_tokens += len(sentence.split());
 *   emit and reset when num_tokens >= target_words; emit the remainder if num_tokens > 0.
 * Whitespace is str.isspace() (the class table of lddl_punkt_set_params, which must have been
 * called); a whitespace-only sentence is skipped. target_words is the reference's
 * target_seq_length - 3 (<= 0: every non-empty sentence is its own chunk).
 * lddl_bart_count: d_sent_off[n_sent+1] (monotone, inside [0, n_bytes], sentences < 2 GiB, cut at
 *   code point boundaries of valid UTF-8), d_doc_sent_off[n_doc+1] (monotone, from 0 to n_sent).
 *   Returns the number of chunks and the bytes of all chunk strings (synchronises the stream).
 *   Exactly one lddl_bart_fill must follow on the same ctx; d_text and both offset arrays must
 *   stay valid until then.
 * lddl_bart_fill -> d_out[n_out_bytes]: the chunk strings back to back (each starts with one
 *   space), d_chunk_off[n_chunks+1] their byte offsets, d_num_tokens[n_chunks] their word counts
 *   (may be NULL), d_doc_chunk_off[n_doc+1] the chunk offsets of the documents. All four NULL
 *   cancels the pending aggregation (releases its scratch).
 * ------------------------------------------------------------------------------------------- */
int lddl_bart_count(lddl_ctx* ctx, void* stream, const uint8_t* d_text, int64_t n_bytes,
                    const int64_t* d_sent_off, int64_t n_sent, const int64_t* d_doc_sent_off,
                    int64_t n_doc, int32_t target_words, int64_t* n_chunks, int64_t* n_out_bytes);
int lddl_bart_fill(lddl_ctx* ctx, void* stream, uint8_t* d_out, int64_t* d_chunk_off,
                   int32_t* d_num_tokens, int64_t* d_doc_chunk_off);

/* ---------------------------------------------------------------------------------------------
 * NSP pairs + static masking for a batch of partitions (device in, device out).
 * Replaces `_to_partition_pairs` (lddl/dask/bert/pretrain.py:386-402) =
 *   for dup in range(duplicate_factor): for doc: create_pairs_from_document(...)  (241-365)
 *     with _truncate_seq_pair (161-176) and, if masking, create_masked_lm_predictions (182-238)
 *   random.shuffle(partition_pairs)
 * after the empty-sentence / empty-document filtering of _get_documents (89-97).
 * Inputs: the tokenizer output (d_ids, d_sent_len) over d_sent_off[n_sent+1];
 *   d_doc_sent_off[n_doc+1] sentence offsets of documents (doc_sent_off[0]=0,
 *   doc_sent_off[n_doc]=n_sent); d_part_doc_off[n_part+1] document offsets of partitions;
 *   d_part_seed[n_part]: rng=LDDL_RNG_REPLAY reproduces CPython `random` after
 *   random.seed(part_seed[p]) bit for bit (vocab_words in id order).
 * lddl_pairs_plan runs the control plane and returns counts[5] = {pairs, tokens (sum of
 * len(A)+len(B)), masked positions, kept sentences, kept documents}; the caller then allocates
 * outputs and calls lddl_pairs_emit. Output pair q (partition order, then the partition shuffle):
 *   tokens[tok_off[q] : tok_off[q] + len_a[q]] = A (masked), then B up to tok_off[q+1];
 *   num_tokens = len(A)+len(B)+3; is_rn[q]; masked positions (sorted, in [CLS] A [SEP] B [SEP]
 *   coordinates) pos[pos_off[q]:pos_off[q+1]] with original-token labels lab[...].
 * params->whole_word = 1 (with masking = 1 and rng = LDDL_RNG_NATIVE; any other combination fails
 *   the call): whole-word masking as Google BERT's do_whole_word_mask. A word is a token that is
 *   no continuation plus the continuations after it; a continuation is a "##x" vocab id that is
 *   not first in A or B and does not follow a literal [CLS]/[SEP]. The pair's words are walked
 *   in a random order and a word is masked iff it still fits the budget (the num_to_predict of
 *   the per-token mode), so a pair has at most that many masked positions, possibly none;
 *   counts[2] and pos_off are exact. The pairs themselves are those of whole_word = 0.
 * ------------------------------------------------------------------------------------------- */
typedef struct lddl_pairs lddl_pairs;
enum { LDDL_RNG_REPLAY = 0, LDDL_RNG_NATIVE = 1 };
typedef struct {
  int32_t seq;            /* --target-seq-length */
  int32_t dup;            /* --duplicate-factor */
  int32_t masking;        /* --masking */
  int32_t rng;            /* LDDL_RNG_REPLAY | LDDL_RNG_NATIVE */
  double short_seq_prob;  /* --short-seq-prob */
  double masked_lm_ratio; /* --masked-lm-ratio */
  uint64_t native_seed;   /* counter-RNG key for LDDL_RNG_NATIVE */
  int32_t whole_word;     /* --whole-word-masking (needs masking and LDDL_RNG_NATIVE) */
} lddl_pair_params;
int lddl_pairs_plan(lddl_ctx* ctx, void* stream, const lddl_pair_params* params,
                    const int64_t* d_sent_off, const int32_t* d_ids, const int32_t* d_sent_len,
                    int64_t n_sent, const int64_t* d_doc_sent_off, int64_t n_doc,
                    const int64_t* d_part_doc_off, const int64_t* d_part_seed, int64_t n_part,
                    lddl_pairs** out, int64_t* counts);
int lddl_pairs_emit(lddl_pairs* plan, void* stream, void* d_tokens, int64_t* d_tok_off,
                    int32_t* d_len_a, uint8_t* d_is_rn, uint16_t* d_pos, void* d_lab,
                    int64_t* d_pos_off);
/* The same plan and gather in two halves, so that the caller's gather of the first partitions'
 * pairs overlaps the planner. With rng = LDDL_RNG_REPLAY and static masking, a batch of more
 * partitions than the device holds planner workgroups is planned in two partition ranges: the
 * head on `stream`, the tail on a side stream of the context (ordered by events only). The pairs
 * of the head are a prefix of the output and final once the head is planned.
 *   lddl_pairs_plan_head: inputs as lddl_pairs_plan. head[8] = {split, head pairs, head tokens,
 *     head masked positions, suggested capacity for pairs, for tokens, for masked positions,
 *     hand-offs of a time-sliced plan (below; 0 when the plan was not sliced)}.
 *     split = 0: the plan is complete and one range; call lddl_pairs_plan_tail for the counts and
 *     lddl_pairs_emit. split = 1: the tail's planner is still running. The capacities are the
 *     head's counts scaled by kept tokens (all) / kept tokens (head) plus a margin: outputs
 *     allocated at them usually hold the whole plan.
 *   lddl_pairs_emit_head: output pairs [0, head pairs) into the caller's buffers (arguments as
 *     lddl_pairs_emit, on the stream of lddl_pairs_plan_head); only between the two plan calls.
 *   lddl_pairs_plan_tail: waits for the tail range, plans its layout and returns counts[5] as
 *     lddl_pairs_plan does. *head_valid = 0 when the head range's output is void: the plan did
 *     not split, or a mask pool overflowed and everything was planned again in one range (the
 *     result is the same; what lddl_pairs_emit_head wrote must be discarded and lddl_pairs_emit
 *     called). Runs on the stream of lddl_pairs_plan_head.
 *   lddl_pairs_emit_tail: output pairs [head pairs, pairs) into the same buffers; needs
 *     *head_valid = 1. The offset tables' entries are absolute, so together the two calls write
 *     exactly what lddl_pairs_emit writes.
 * lddl_pairs_plan = lddl_pairs_plan_head + lddl_pairs_plan_tail. LDDL_PLAN_SPLIT (environment,
 * A/B): unset or -1 = automatic, 0 = never split, k > 0 = a head of exactly min(k, n_part)
 * partitions; any other value fails the call.
 * (Automatic: never, since a batch of more partitions than the device holds planner workgroups
 * is time-sliced instead, below; the split plan runs when LDDL_PLAN_SPLIT forces it, or with
 * LDDL_PLAN_SLICE=0.)
 * LDDL_PLAN_SLICE (environment, A/B): the time-sliced replay plan, one range planned by as many
 * persistent planner waves as the device holds, each working on a partition for a quantum of
 * documents before it parks it and takes the next from a queue. Unset or -1 = automatic, 0 =
 * never, k > 0 = always, with a quantum of k documents; any other value fails the call, and so
 * does a positive value together with a positive LDDL_PLAN_SPLIT (a split plan is not sliced).
 * LDDL_PLAN_WAVES = g >= 1 overrides the number of persistent waves. */
int lddl_pairs_plan_head(lddl_ctx* ctx, void* stream, const lddl_pair_params* params,
                         const int64_t* d_sent_off, const int32_t* d_ids, const int32_t* d_sent_len,
                         int64_t n_sent, const int64_t* d_doc_sent_off, int64_t n_doc,
                         const int64_t* d_part_doc_off, const int64_t* d_part_seed, int64_t n_part,
                         lddl_pairs** out, int64_t* head);
int lddl_pairs_emit_head(lddl_pairs* plan, void* stream, void* d_tokens, int64_t* d_tok_off,
                         int32_t* d_len_a, uint8_t* d_is_rn, uint16_t* d_pos, void* d_lab,
                         int64_t* d_pos_off);
int lddl_pairs_plan_tail(lddl_pairs* plan, int64_t* counts, int32_t* head_valid);
int lddl_pairs_emit_tail(lddl_pairs* plan, void* stream, void* d_tokens, int64_t* d_tok_off,
                         int32_t* d_len_a, uint8_t* d_is_rn, uint16_t* d_pos, void* d_lab,
                         int64_t* d_pos_off);
int lddl_pairs_destroy(lddl_pairs* plan, void* stream);
/* d_part_pair_off[n_part + 1]: first output pair of each partition (pairs are emitted in
 * partition order), i.e. the row ranges of the reference's per-partition outputs. */
int lddl_pairs_part_offsets(lddl_pairs* plan, void* stream, int64_t* d_part_pair_off);
/* Device time (ms, HIP events on the plan's stream) of the planner kernel of lddl_pairs_plan:
 * from its first launch until its last partition range is complete (a split plan: after
 * lddl_pairs_plan_tail; the span includes what ran on the stream under the tail range). */
int lddl_pairs_plan_ms(const lddl_pairs* plan, float* ms);

/* ---------------------------------------------------------------------------------------------
 * Per-partition sequence-length binning.
 * Replaces _to_dataframe_binned (lddl/dask/bert/binning.py:63-93) applied per partition:
 *   bin_id = min((num_tokens - 1) // bin_size, nbins - 1), rows regrouped by bin, stable.
 * Rows of partition p are d_part_off[p] .. d_part_off[p+1]; row r's num_tokens is d_num_tokens[r],
 * or, with d_num_tokens NULL, d_tok_off[r+1] - d_tok_off[r] + 3 (a lddl_pairs_emit offset table).
 * Outputs (device, every entry written): d_perm[r] = input
 * row of output row r (partition order kept, bins ascending inside a partition), d_bin_id[r] its
 * bin, d_counts[p * nbins + b] = rows of partition p in bin b. nbins <= 8192.
 * ------------------------------------------------------------------------------------------- */
int lddl_bin_partitions(lddl_ctx* ctx, void* stream, const int32_t* d_num_tokens,
                        const int64_t* d_tok_off, int64_t n_rows, const int64_t* d_part_off,
                        int64_t n_part, int32_t bin_size, int32_t nbins, int64_t* d_perm,
                        int64_t* d_bin_id, int64_t* d_counts);

/* The same regroup for ONE large segment (a rank's rows of one batch before the load-balance
 * exchange), spread over many workgroups: d_perm / d_bin_id (may be NULL) as above, d_counts[b]
 * rows per bin. num_tokens of row r = d_num_tokens[r], or, with d_num_tokens NULL, the pair's
 * token count + 3 from a lddl_pairs_emit offset table: d_tok_off[r+1] - d_tok_off[r] + 3. */
int lddl_bin_stable(lddl_ctx* ctx, void* stream, const int32_t* d_num_tokens,
                    const int64_t* d_tok_off, int64_t n_rows, int32_t bin_size, int32_t nbins,
                    int64_t* d_perm, int64_t* d_bin_id, int64_t* d_counts);

/* ---------------------------------------------------------------------------------------------
 * Rendering of the parquet columns (lddl/dask/bert/pretrain.py:345-358):
 *   A, B = ' '.join(tokens), masked_lm_labels = ' '.join(labels) (vocab strings of the ids),
 *   masked_lm_positions = np.save bytes of uint16[k] (lddl/utils.py:98-102; 128 + 2k bytes).
 * Output row r renders pair d_rows[r] (d_rows NULL = identity) of a lddl_pairs_emit table.
 * lddl_render_lengths writes per-row byte lengths; the caller scans them (lddl_scan_i64) into
 * offsets and calls lddl_render_write. Label / position arguments may be NULL (no masking).
 * It also writes the rows' num_tokens (uint16, len(A) + len(B) + 3) and, from d_is_rn,
 * is_random_next in output order (each output pointer may be NULL).
 * ------------------------------------------------------------------------------------------- */
int lddl_render_lengths(lddl_ctx* ctx, void* stream, const void* d_tokens,
                        const int64_t* d_tok_off, const int32_t* d_len_a, const void* d_lab,
                        const int64_t* d_pos_off, const int64_t* d_rows, int64_t n_rows,
                        int64_t* d_a_len, int64_t* d_b_len, int64_t* d_l_len, int64_t* d_npy_len,
                        const uint8_t* d_is_rn, uint16_t* d_num_tokens_out, uint8_t* d_is_rn_out);
int lddl_render_write(lddl_ctx* ctx, void* stream, const void* d_tokens,
                      const int64_t* d_tok_off, const int32_t* d_len_a, const uint16_t* d_pos,
                      const void* d_lab, const int64_t* d_pos_off, const int64_t* d_rows,
                      int64_t n_rows, const int64_t* d_a_off, const int64_t* d_b_off,
                      const int64_t* d_l_off, const int64_t* d_npy_off, uint8_t* d_a_bytes,
                      uint8_t* d_b_bytes, uint8_t* d_l_bytes, uint8_t* d_npy_bytes);

/* ---------------------------------------------------------------------------------------------
 * Row movement of the load balance (lddl_amd/balance.py; replaces the reference's filesystem
 * shuffle, lddl/dask/load_balance.py:84-156). Rows are addressed over TWO sources: row r < n_a is
 * row r of source A, else row r - n_a of source B (B may be NULL when every r < n_a); d_rows NULL
 * = the identity (n_rows <= n_a). elem_bytes in {1, 2, 4, 8}; offsets count elements and are
 * relative to their own source.
 *   lddl_gather_ragged: elements src[off[r] .. off[r+1]) of output row i (r = d_rows[i]) copied to
 *     d_dst[d_dst_off[i] ...].
 *   lddl_take: d_dst[i] = src[r].
 *   lddl_ragged_offsets: d_out[0..n_rows] = exclusive scan of the rows' sizes off[r+1] - off[r].
 *   lddl_expand_segments: segment k covers d_out[seg_off[k] .. seg_off[k+1]); its element t is
 *     v = seg[3k] + t * seg[3k+1], written as v when seg[3k+2] != 0, else as d_src[v]
 *     (the balance plan's strided row runs, expanded on the device).
 *   lddl_pairs_meta_pack: int32[n][4] {len(A)+len(B), len(A), is_random_next, masks} of rows d_rows
 *     of a pair table (d_pos_off NULL: 0 masks); lddl_pairs_meta_unpack splits it into columns
 *     (d_nmask may be NULL).
 * ------------------------------------------------------------------------------------------- */
int lddl_gather_ragged(void* stream, const void* d_src_a, const int64_t* d_off_a, int64_t n_a,
                       const void* d_src_b, const int64_t* d_off_b, int32_t elem_bytes,
                       const int64_t* d_rows, int64_t n_rows, const int64_t* d_dst_off, void* d_dst);
int lddl_take(void* stream, const void* d_a, int64_t n_a, const void* d_b, int32_t elem_bytes,
              const int64_t* d_rows, int64_t n_rows, void* d_dst);
int lddl_ragged_offsets(lddl_ctx* ctx, void* stream, const int64_t* d_off_a, int64_t n_a,
                        const int64_t* d_off_b, const int64_t* d_rows, int64_t n_rows,
                        int64_t* d_out);
int lddl_expand_segments(void* stream, const int64_t* d_src, const int64_t* d_seg,
                         const int64_t* d_seg_off, int64_t n_seg, int64_t total, int64_t* d_out);
int lddl_pairs_meta_pack(void* stream, const int64_t* d_tok_off, const int32_t* d_len_a,
                         const uint8_t* d_is_rn, const int64_t* d_pos_off, const int64_t* d_rows,
                         int64_t n, int32_t* d_meta);
int lddl_pairs_meta_unpack(void* stream, const int32_t* d_meta, int64_t n, int64_t* d_ntok,
                           int32_t* d_len_a, uint8_t* d_is_rn, int64_t* d_nmask);

/* Exclusive prefix sum: d_out[0..n] (d_out[n] = total) of d_in[0..n) (scratch from the ctx). */
int lddl_scan_i64(lddl_ctx* ctx, void* stream, const int64_t* d_in, int64_t n, int64_t* d_out);

/* ---------------------------------------------------------------------------------------------
 * Loader collate (lddl/torch/bert.py:69-149 `_to_encoded_inputs`), one batch, device in/out.
 *   d_bytes: A / B strings of the batch (space-joined tokens, as stored in the parquet shards);
 *   sample b: A = d_bytes[a_off[b], a_off[b+1]), B = d_bytes[b_off[b], b_off[b+1]);
 *   d_na/d_nb: token counts; seq_len = roundup(max(na+nb+3), sequence_length_alignment).
 *   Outputs int64 [batch, seq_len]: input_ids (convert_tokens_to_ids, [UNK] if absent),
 *   token_type_ids, attention_mask, and either special_tokens_mask (dynamic masking) or labels
 *   (static: d_lab_bytes/d_lab_off = masked_lm_labels strings, d_pos/d_pos_off = decoded
 *   masked_lm_positions; unmasked slots = ignore_index). Unused outputs may be NULL.
 *   Token and label writes at positions >= seq_len are dropped (the host refuses such a batch
 *   with IndexError before launching, as the reference's tensor indexing does).
 * ------------------------------------------------------------------------------------------- */
int lddl_collate_encode(lddl_ctx* ctx, void* stream, const uint8_t* d_bytes, const int64_t* d_a_off,
                        const int64_t* d_b_off, const int32_t* d_na, const int32_t* d_nb,
                        int32_t batch, int32_t seq_len, int64_t* d_input_ids,
                        int64_t* d_token_type_ids, int64_t* d_attention_mask,
                        int64_t* d_special_tokens_mask, const uint8_t* d_lab_bytes,
                        const int64_t* d_lab_off, const uint16_t* d_pos, const int64_t* d_pos_off,
                        int64_t* d_labels, int64_t ignore_index);

/* The static-masking collate of the model-parallel loader (lddl/torch_mp/bert.py:69-153): as
 * lddl_collate_encode, plus d_loss_mask int64 [batch, seq_len] = 1 at the sample's
 * masked_lm_positions (duplicates included, whatever the labels string holds), else 0; written
 * by the same kernel in the same pass. Fails with -1 before anything is launched if d_loss_mask,
 * d_labels or a static-masking input (d_lab_bytes, d_lab_off, d_pos, d_pos_off) is NULL. The
 * other outputs are bit-identical to lddl_collate_encode's. */
int lddl_collate_encode_mp(lddl_ctx* ctx, void* stream, const uint8_t* d_bytes,
                           const int64_t* d_a_off, const int64_t* d_b_off, const int32_t* d_na,
                           const int32_t* d_nb, int32_t batch, int32_t seq_len,
                           int64_t* d_input_ids, int64_t* d_token_type_ids,
                           int64_t* d_attention_mask, int64_t* d_special_tokens_mask,
                           const uint8_t* d_lab_bytes, const int64_t* d_lab_off,
                           const uint16_t* d_pos, const int64_t* d_pos_off, int64_t* d_labels,
                           int64_t ignore_index, int64_t* d_loss_mask);

/* The loader's dynamic-masking collate in one pass (lddl/torch/bert.py:348-365 =
 * _to_encoded_inputs + _mask_tokens): as lddl_collate_encode (dynamic), then the native-RNG
 * masking of lddl_mask_dynamic applied to each slot as it is written; outputs input_ids (masked),
 * token_type_ids, attention_mask, labels. Bit-identical to lddl_collate_encode followed by
 * lddl_mask_dynamic with the same seed / counter. */
int lddl_collate_encode_masked(lddl_ctx* ctx, void* stream, const uint8_t* d_bytes,
                               const int64_t* d_a_off, const int64_t* d_b_off, const int32_t* d_na,
                               const int32_t* d_nb, int32_t batch, int32_t seq_len,
                               int64_t* d_input_ids, int64_t* d_token_type_ids,
                               int64_t* d_attention_mask, int64_t* d_labels, float mlm_probability,
                               int64_t ignore_index, int64_t vocab_len, uint64_t seed,
                               uint64_t counter);

/* ---------------------------------------------------------------------------------------------
 * Dynamic masking (lddl/torch/bert.py:152-196 `_mask_tokens`) in place on d_input_ids
 * [batch, seq_len] int64; writes d_labels. Special slots come from d_special_tokens_mask, or,
 * if NULL, from the lengths (positions 0, na+1 and >= na+nb+2, as _to_encoded_inputs sets them),
 * or, if the lengths are NULL too, from the ids: a slot is special iff its id is one of
 * [PAD] [UNK] [CLS] [SEP] [MASK] (`special_tokens_mask=None`, i.e.
 * tokenizer.get_special_tokens_mask(ids, already_has_special_tokens=True), bert.py:167-172).
 * Native mode: Philox4x32-10 keyed by (seed, counter) — call with a fresh counter per batch.
 * Replay mode (all four d_r_* non-NULL): apply captured torch draws (masked_indices,
 * indices_replaced, indices_random as uint8, random_words int64) bit for bit.
 * ------------------------------------------------------------------------------------------- */
int lddl_mask_dynamic(lddl_ctx* ctx, void* stream, int64_t* d_input_ids, int64_t* d_labels,
                      const int64_t* d_special_tokens_mask, const int32_t* d_na, const int32_t* d_nb,
                      int64_t batch, int64_t seq_len, float mlm_probability, int64_t ignore_index,
                      int64_t vocab_len, uint64_t seed, uint64_t counter,
                      const uint8_t* d_r_masked, const uint8_t* d_r_replaced,
                      const uint8_t* d_r_random, const int64_t* d_r_words);

/* ---------------------------------------------------------------------------------------------
 * Whole-word dynamic masking (Google BERT's do_whole_word_mask; past the reference). A slot is a
 * continuation iff it is not special, is not the row's first slot, the slot before it is not
 * special, and its id is a continuation id: 0 <= id < vocab size of the context and the vocab
 * line starts with "##" and is longer than 2 bytes (decided from the id, never from a string).
 * head(x) = the largest h <= x that is not a continuation. With r(i) the Philox output that
 * lddl_mask_dynamic draws for flat slot i (same seed / counter):
 *   masked(x) = !special(x) && u01(r(head(x)).x) < mlm_probability;
 * 80 / 10 / 10 and the random id come from the slot's own r(x).y/.z/.w, labels as before. A row
 * without continuation ids comes out bit-identical to the plain entry point's.
 *
 * lddl_mask_dynamic_ww: lddl_mask_dynamic's native mode (no replay). One wave per row.
 * lddl_collate_encode_masked_ww: lddl_collate_encode_masked with the whole-word decision;
 * bit-identical to lddl_collate_encode followed by lddl_mask_dynamic_ww.
 * Both fail with -1 on a NULL context or a vocab without [MASK].
 * ------------------------------------------------------------------------------------------- */
int lddl_mask_dynamic_ww(lddl_ctx* ctx, void* stream, int64_t* d_input_ids, int64_t* d_labels,
                         const int64_t* d_special_tokens_mask, const int32_t* d_na,
                         const int32_t* d_nb, int64_t batch, int64_t seq_len,
                         float mlm_probability, int64_t ignore_index, int64_t vocab_len,
                         uint64_t seed, uint64_t counter);

int lddl_collate_encode_masked_ww(lddl_ctx* ctx, void* stream, const uint8_t* d_bytes,
                                  const int64_t* d_a_off, const int64_t* d_b_off,
                                  const int32_t* d_na, const int32_t* d_nb, int32_t batch,
                                  int32_t seq_len, int64_t* d_input_ids, int64_t* d_token_type_ids,
                                  int64_t* d_attention_mask, int64_t* d_labels,
                                  float mlm_probability, int64_t ignore_index, int64_t vocab_len,
                                  uint64_t seed, uint64_t counter);

/* ---------------------------------------------------------------------------------------------
 * Sequence-packed collate (past the reference): several samples share one row of
 * max_seq_length slots. The host plans the rows; per sample i (len = na + nb + 3):
 *   d_dst[i]         flat slot row * max_seq_length + start of the sample's [CLS]
 *   d_fill[i]        slots its wave writes: len, plus the row's unused tail if it is the row's
 *                    last sample. The segments [dst, dst + fill) must tile the [R, L] outputs:
 *                    every element is then written exactly once (no memset needed)
 *   d_seq_in_row[i]  1-based index of the sample inside its row
 * Outputs, all [R, max_seq_length] int64: slot x < len of the segment holds what the unpacked
 * entry point puts at [i, x], position_ids = x and sequence_ids = seq_in_row; slots
 * [len, fill) are padding: input_ids, token_type_ids, attention_mask, position_ids and
 * sequence_ids 0, labels ignore_index, special_tokens_mask 1. A sample with
 * len > max_seq_length is not written (the host refuses it).
 *
 * lddl_collate_seqpack: lddl_collate_encode. Static masking (d_lab_bytes given: positions count
 * from the sample's [CLS], one >= len is dropped; writes d_labels, d_special_tokens_mask NULL)
 * or dynamic unmasked (d_lab_bytes NULL: writes d_special_tokens_mask, d_labels NULL).
 * lddl_collate_seqpack_masked: lddl_collate_encode_masked, or with whole_word != 0
 * lddl_collate_encode_masked_ww (64-slot windows from the sample's start). The Philox index of
 * slot x of sample i is i * draw_stride + x: with draw_stride = the seq_len of the unpacked call
 * and equal seed / counter, the segment is bit-identical to row i of the unpacked output.
 * Both fail with -1 on a NULL context, a NULL output or plan array, a vocab without [CLS] and
 * [SEP] (masked: and [MASK]), or max_seq_length too long for the kernel's LDS staging.
 * ------------------------------------------------------------------------------------------- */
int lddl_collate_seqpack(lddl_ctx* ctx, void* stream, const uint8_t* d_bytes,
                         const int64_t* d_a_off, const int64_t* d_b_off, const int32_t* d_na,
                         const int32_t* d_nb, int32_t batch, const int64_t* d_dst,
                         const int32_t* d_fill, const int32_t* d_seq_in_row,
                         int32_t max_seq_length, int64_t* d_input_ids, int64_t* d_token_type_ids,
                         int64_t* d_attention_mask, int64_t* d_special_tokens_mask,
                         const uint8_t* d_lab_bytes, const int64_t* d_lab_off,
                         const uint16_t* d_pos, const int64_t* d_pos_off, int64_t* d_labels,
                         int64_t ignore_index, int64_t* d_position_ids, int64_t* d_sequence_ids);

int lddl_collate_seqpack_masked(lddl_ctx* ctx, void* stream, const uint8_t* d_bytes,
                                const int64_t* d_a_off, const int64_t* d_b_off,
                                const int32_t* d_na, const int32_t* d_nb, int32_t batch,
                                const int64_t* d_dst, const int32_t* d_fill,
                                const int32_t* d_seq_in_row, int32_t max_seq_length,
                                int32_t draw_stride, int64_t* d_input_ids,
                                int64_t* d_token_type_ids, int64_t* d_attention_mask,
                                int64_t* d_labels, int64_t* d_position_ids,
                                int64_t* d_sequence_ids, float mlm_probability,
                                int64_t ignore_index, int64_t vocab_len, uint64_t seed,
                                uint64_t counter, int32_t whole_word);

/* ---------------------------------------------------------------------------------------------
 * Collate from a pair table (past the reference: the online loader, lddl_amd/torch/online.py).
 * The input is a lddl_pairs_emit table, ids of lddl_ctx_id_bytes() bytes: pair q has A =
 * d_tokens[tok_off[q], tok_off[q] + len_a[q]), B = the rest up to tok_off[q+1], and with static
 * masking the positions d_pos[pos_off[q], pos_off[q+1]) ([CLS] A [SEP] B [SEP] coordinates) with
 * the original ids d_lab at the same indices. Output row i is pair d_rows[i] (d_rows NULL = the
 * identity); outputs int64 [batch, seq_len], d_next_sentence_labels int64 [batch] = is_rn.
 *
 * The outputs are bit-identical to what the string entry points write for the strings
 * lddl_render_write makes of the same pairs in the same order, with equal seq_len, seed and
 * counter (the Philox index of slot x of row i is i * seq_len + x), for every vocab in which no
 * two lines hold the same string:
 *   lddl_collate_pairs         lddl_collate_encode. Static masking (d_pos, d_lab, d_pos_off given:
 *                              writes d_labels, unmasked slots = ignore_index; a position >=
 *                              seq_len is dropped, the host refuses it with IndexError) or none
 *                              (all three NULL: writes d_special_tokens_mask). The output that is
 *                              not written may be NULL.
 *   lddl_collate_pairs_masked  lddl_collate_encode_masked, or with whole_word != 0
 *                              lddl_collate_encode_masked_ww.
 * A pair longer than seq_len is refused on the host (ValueError); on the device its slots past
 * the row are not written. One wave per row, 64-bit offsets, every output element written once.
 * batch <= 0 returns 0. Both fail with -1 before anything is launched on a NULL context, a NULL
 * table array or required output, static inputs given in part, or a vocab without [CLS] and
 * [SEP] (masked: and [MASK]).
 * ------------------------------------------------------------------------------------------- */
int lddl_collate_pairs(lddl_ctx* ctx, void* stream, const void* d_tokens, const int64_t* d_tok_off,
                       const int32_t* d_len_a, const uint8_t* d_is_rn, const uint16_t* d_pos,
                       const void* d_lab, const int64_t* d_pos_off, const int64_t* d_rows,
                       int32_t batch, int32_t seq_len, int64_t* d_input_ids,
                       int64_t* d_token_type_ids, int64_t* d_attention_mask,
                       int64_t* d_special_tokens_mask, int64_t* d_labels,
                       int64_t* d_next_sentence_labels, int64_t ignore_index);

int lddl_collate_pairs_masked(lddl_ctx* ctx, void* stream, const void* d_tokens,
                              const int64_t* d_tok_off, const int32_t* d_len_a,
                              const uint8_t* d_is_rn, const int64_t* d_rows, int32_t batch,
                              int32_t seq_len, int64_t* d_input_ids, int64_t* d_token_type_ids,
                              int64_t* d_attention_mask, int64_t* d_labels,
                              int64_t* d_next_sentence_labels, float mlm_probability,
                              int64_t ignore_index, int64_t vocab_len, uint64_t seed,
                              uint64_t counter, int32_t whole_word);

/* ---------------------------------------------------------------------------------------------
 * The row plan of sequence packing, made on the device (past the reference: the packed online
 * loader). For every batch it computes exactly what lddl_amd/torch/seqpack.py's
 * plan_rows(lengths, capacity) computes: first-fit decreasing, samples visited by length
 * descending (ties: the lower index within the batch first), each into the lowest-numbered open
 * row with room, else into a new row; samples sit back to back in a row in the order placed.
 *
 * Batch k is the samples d_rows[d_batch_off[k] .. d_batch_off[k+1]) (d_rows NULL = the
 * identity); the batches tile [0, n_rows). The length of sample i is d_num_tokens[r], r =
 * rows[i], or, with d_num_tokens NULL, d_tok_off[r+1] - d_tok_off[r] + 3 (lddl_bin_stable's
 * convention). Every r must be a row of that array. Outputs, indexed like d_rows, every entry
 * written:
 *   d_dst[i]         row * capacity + start, relative to the batch's own [R, capacity] output
 *   d_fill[i]        the sample's length; the last sample placed into a row also gets the row's
 *                    unused tail
 *   d_seq_in_row[i]  1-based index of the sample in its row
 *   d_packed_idx[i]  position of the sample in (row, start) order = plan_rows' order^-1
 *   d_num_rows[k]    R of batch k (an empty batch: 0)
 * A sample longer than capacity takes no row: dst = -1, fill = 0, seq_in_row = 0, packed_idx =
 * -1, and the rest of the batch is planned as if it were not there.
 *
 * One wave per batch, all batches in one launch, no host wait. A batch holds at most
 * LDDL_SEQPLAN_MAX_BATCH samples. Fails with -1 before anything is launched on a NULL context,
 * a NULL output or d_batch_off, both length sources NULL, capacity < 1, or n_rows >
 * n_batches * LDDL_SEQPLAN_MAX_BATCH (some batch is then too large: with one batch this is the
 * exact test). The offsets themselves are device memory, which the host does not wait for: a
 * larger batch that this test cannot see is marked on the device (d_num_rows[k] = -1, its
 * samples take no row), and a range outside [0, n_rows) writes only d_num_rows[k] = -1.
 * n_batches <= 0 returns 0.
 * ------------------------------------------------------------------------------------------- */
#define LDDL_SEQPLAN_MAX_BATCH 1024
int lddl_seqpack_plan(lddl_ctx* ctx, void* stream, const int32_t* d_num_tokens,
                      const int64_t* d_tok_off, const int64_t* d_rows, int64_t n_rows,
                      const int64_t* d_batch_off, int32_t n_batches, int32_t capacity,
                      int64_t* d_dst, int32_t* d_fill, int32_t* d_seq_in_row,
                      int32_t* d_packed_idx, int32_t* d_num_rows);

/* ---------------------------------------------------------------------------------------------
 * Sequence-packed collate from a pair table (past the reference): to
 * lddl_collate_seqpack[_masked] what lddl_collate_pairs[_masked] is to
 * lddl_collate_encode[_masked]. The table and d_rows are lddl_collate_pairs'; d_dst, d_fill,
 * d_seq_in_row and d_packed_idx are the plan of these `batch` samples (lddl_seqpack_plan's
 * arrays from the batch's first sample on, or a host plan), out_rows its R.
 *
 * Outputs [out_rows, max_seq_length] int64: slot x < len of sample i's segment
 * [dst[i], dst[i] + fill[i]) holds what lddl_collate_pairs[_masked] puts at [i, x], plus
 * position_ids = x and sequence_ids = seq_in_row[i]; slots [len, fill) are padding with
 * lddl_collate_seqpack's values. Per sample, at packed_idx[i]: d_next_sentence_labels (int64),
 * d_cls_positions (int64, = dst[i]) and d_seq_lens (int32, = len). Every output element is
 * written once by a plan whose segments tile the outputs. A sample whose segment does not lie
 * inside the outputs, or with dst < 0, fill < len, len > max_seq_length, seq_in_row < 1 or
 * packed_idx outside [0, batch), writes nothing.
 *
 *   lddl_collate_pairs_seqpack         static masking (d_pos, d_lab, d_pos_off: positions count
 *                                      from the sample's [CLS], one >= len is dropped, the host
 *                                      refuses it with IndexError; writes d_labels) or none (all
 *                                      three NULL: writes d_special_tokens_mask)
 *   lddl_collate_pairs_seqpack_masked  dynamic masking, per token or (whole_word != 0) whole
 *                                      words in 64-slot windows from the sample's start. The
 *                                      Philox index of slot x of sample i is i * draw_stride + x:
 *                                      with draw_stride = the seq_len of lddl_collate_pairs_masked
 *                                      and equal seed / counter the segment is bit-identical to
 *                                      row i of its output.
 * batch, out_rows or max_seq_length <= 0 returns 0. Both fail with -1 before anything is
 * launched on a NULL context, a NULL table array, plan array or required output, static inputs
 * given in part, a vocab without [CLS] and [SEP] (masked: and [MASK]), or (static masking)
 * max_seq_length too long for the kernel's LDS staging.
 * ------------------------------------------------------------------------------------------- */
int lddl_collate_pairs_seqpack(lddl_ctx* ctx, void* stream, const void* d_tokens,
                               const int64_t* d_tok_off, const int32_t* d_len_a,
                               const uint8_t* d_is_rn, const uint16_t* d_pos, const void* d_lab,
                               const int64_t* d_pos_off, const int64_t* d_rows, int32_t batch,
                               const int64_t* d_dst, const int32_t* d_fill,
                               const int32_t* d_seq_in_row, const int32_t* d_packed_idx,
                               int32_t out_rows, int32_t max_seq_length, int64_t* d_input_ids,
                               int64_t* d_token_type_ids, int64_t* d_attention_mask,
                               int64_t* d_special_tokens_mask, int64_t* d_labels,
                               int64_t* d_position_ids, int64_t* d_sequence_ids,
                               int64_t* d_next_sentence_labels, int64_t* d_cls_positions,
                               int32_t* d_seq_lens, int64_t ignore_index);

int lddl_collate_pairs_seqpack_masked(lddl_ctx* ctx, void* stream, const void* d_tokens,
                                      const int64_t* d_tok_off, const int32_t* d_len_a,
                                      const uint8_t* d_is_rn, const int64_t* d_rows, int32_t batch,
                                      const int64_t* d_dst, const int32_t* d_fill,
                                      const int32_t* d_seq_in_row, const int32_t* d_packed_idx,
                                      int32_t out_rows, int32_t max_seq_length,
                                      int32_t draw_stride, int64_t* d_input_ids,
                                      int64_t* d_token_type_ids, int64_t* d_attention_mask,
                                      int64_t* d_labels, int64_t* d_position_ids,
                                      int64_t* d_sequence_ids, int64_t* d_next_sentence_labels,
                                      int64_t* d_cls_positions, int32_t* d_seq_lens,
                                      float mlm_probability, int64_t ignore_index,
                                      int64_t vocab_len, uint64_t seed, uint64_t counter,
                                      int32_t whole_word);

/* ---------------------------------------------------------------------------------------------
 * N-gram (span) dynamic masking (past the reference): whole words as above, masked in
 * runs of up to n words, as Megatron-LM's BERT dataset, ALBERT and SpanBERT mask them. special(x),
 * the continuation test and "head" are those of the whole-word entry points. Per row:
 *   word(x) = #{y <= x : !special(y) && !continuation(y)} - 1 for a non-special slot x; special
 *     slots are no words, are never masked and do not stop a span (A's last word and B's first
 *     are neighbours);
 *   a non-special head h of word j starts a span iff u01(r(h).x) < p_start, r the draw of
 *     lddl_mask_dynamic at the same flat index, seed and counter; its length in words is
 *     len(h) = 1 + #{k in [1, n) : u01(r2(h).x) >= cum[k - 1]}, r2 the same Philox call under
 *     the key seed ^ LDDL_SPAN_SEED_XOR; its reach e(j) = j + len(h), and 0 without a start;
 *   masked(x) = !special(x) && max_{j' <= word(x)} e(j') > word(x): overlapping spans merge, a
 *     span runs on over special slots and ends with the row; there is no budget per row;
 *   80 / 10 / 10 and the random id come from the slot's own r(x).y/.z/.w, labels as before.
 * n = 1 is bit-identical to the whole-word entry points. A word with n - 1 words before it is
 * masked with probability mlm_probability; the first n - 1 words of a row have fewer words
 * before them and are masked slightly less often.
 *
 * lddl_span_params_make (host only): P(len = k) = weights[k - 1], k = 1..n, or with weights NULL
 * proportional to 1 / k (ALBERT, Google BERT's ngram masking); cum[k - 1] = float(P(len <= k)) for
 * k < n and 1 from there on; p_start solves 1 - prod_{k < n} (1 - s * P(len > k)) =
 * mlm_probability (in double, then cast; for n = 1 it is (float)mlm_probability). Fails with -1
 * on n outside [1, LDDL_SPAN_MAX_N], a negative weight, weights that do not sum to 1 within
 * 1e-9, mlm_probability outside [0, 1], or out NULL.
 *
 * The five entry points take the arguments of their whole-word siblings (without the whole_word
 * flag) and the params; the kernels read params->p_start where the siblings read
 * mlm_probability, which is kept for the callers' bookkeeping. The packed ones keep the
 * per-sample state and the draw_stride index: a sample's segment is bit-identical to its row in
 * the unpacked output. Each equals its two-pass form (the unmasked collate, then
 * lddl_mask_dynamic_span). Each fails with -1 before anything is launched in its sibling's cases
 * and on NULL params or params that lddl_span_params_make cannot have written.
 * ------------------------------------------------------------------------------------------- */
#define LDDL_SPAN_MAX_N 16
#define LDDL_SPAN_SEED_XOR 0x9E3779B97F4A7C15ull
typedef struct {
  int32_t n;                        /* longest span, in words */
  float p_start;                    /* a head starts a span with this probability */
  float cum[LDDL_SPAN_MAX_N - 1];   /* cum[k - 1] = P(len <= k) for k < n, 1 from there on */
} lddl_span_params;

int lddl_span_params_make(double mlm_probability, int32_t n, const double* weights,
                          lddl_span_params* out);

/* N-gram (span) static masking in the pair planner (past the reference):
 * lddl_pairs_plan_head with one more argument. span = NULL is lddl_pairs_plan_head. Otherwise
 * params->masking = 1 and params->rng = LDDL_RNG_NATIVE are needed and span must be one that
 * lddl_span_params_make can have written (n and cum are read, p_start is not); any other case
 * fails with -1 and a message naming span, before anything is allocated or launched.
 * params->whole_word beside it changes nothing. Tail, emit, destroy and part offsets are the
 * existing calls.
 *   Words, specials, continuations and the budget (the per-token mode's num_to_predict) are
 *   those of whole_word = 1; the words 0 .. W - 1 are numbered in token order. An n-gram is n
 *   consecutive words j .. j + n - 1; it may run from A into B and over a literal [CLS]/[SEP],
 *   which is never masked and does not count: tok(j, n) = the non-special tokens of those words.
 *   Head h (a token index) of planner pair idx draws from its whole-word key block: the first
 *   word is the order key, the second, y, the length
 *     L(h) = 1 + #{k in [1, n) : u01(y) >= cum[k - 1]}.
 *   The words are visited in the whole-word order (key, then token index mod 64, then token
 *   index), each once, with masked = 0 and nothing covered at the start. For a visited word j:
 *   stop if masked = budget; n = min(L(head_j), W - j) (clipped at the pair's end, not
 *   renormalised); while n >= 1 and masked + tok(j, n) > budget, n -= 1; if n = 0, or any of the
 *   words j .. j + n - 1 is covered (j itself included), go on to the next word (the start is
 *   dropped, not shrunk); else cover them, mask their tokens and add tok(j, n) to masked.
 *   80 / 10 / 10 and the random id come from the token's own decide block, as with whole_word.
 * A pair may end below its budget, also at 0; counts[2] and pos_off are exact. n = 1 is
 * bit-identical to whole_word = 1, and the pairs themselves are those of the per-token run.
 * Not built: favor_longer_ngram, and length weights renormalised per start. */
int lddl_pairs_plan_head_span(lddl_ctx* ctx, void* stream, const lddl_pair_params* params,
                              const int64_t* d_sent_off, const int32_t* d_ids,
                              const int32_t* d_sent_len, int64_t n_sent,
                              const int64_t* d_doc_sent_off, int64_t n_doc,
                              const int64_t* d_part_doc_off, const int64_t* d_part_seed,
                              int64_t n_part, lddl_pairs** out, int64_t* head,
                              const lddl_span_params* span);

int lddl_mask_dynamic_span(lddl_ctx* ctx, void* stream, int64_t* d_input_ids, int64_t* d_labels,
                           const int64_t* d_special_tokens_mask, const int32_t* d_na,
                           const int32_t* d_nb, int64_t batch, int64_t seq_len,
                           float mlm_probability, int64_t ignore_index, int64_t vocab_len,
                           uint64_t seed, uint64_t counter, const lddl_span_params* params);

int lddl_collate_encode_masked_span(lddl_ctx* ctx, void* stream, const uint8_t* d_bytes,
                                    const int64_t* d_a_off, const int64_t* d_b_off,
                                    const int32_t* d_na, const int32_t* d_nb, int32_t batch,
                                    int32_t seq_len, int64_t* d_input_ids,
                                    int64_t* d_token_type_ids, int64_t* d_attention_mask,
                                    int64_t* d_labels, float mlm_probability,
                                    int64_t ignore_index, int64_t vocab_len, uint64_t seed,
                                    uint64_t counter, const lddl_span_params* params);

int lddl_collate_seqpack_masked_span(lddl_ctx* ctx, void* stream, const uint8_t* d_bytes,
                                     const int64_t* d_a_off, const int64_t* d_b_off,
                                     const int32_t* d_na, const int32_t* d_nb, int32_t batch,
                                     const int64_t* d_dst, const int32_t* d_fill,
                                     const int32_t* d_seq_in_row, int32_t max_seq_length,
                                     int32_t draw_stride, int64_t* d_input_ids,
                                     int64_t* d_token_type_ids, int64_t* d_attention_mask,
                                     int64_t* d_labels, int64_t* d_position_ids,
                                     int64_t* d_sequence_ids, float mlm_probability,
                                     int64_t ignore_index, int64_t vocab_len, uint64_t seed,
                                     uint64_t counter, const lddl_span_params* params);

int lddl_collate_pairs_masked_span(lddl_ctx* ctx, void* stream, const void* d_tokens,
                                   const int64_t* d_tok_off, const int32_t* d_len_a,
                                   const uint8_t* d_is_rn, const int64_t* d_rows, int32_t batch,
                                   int32_t seq_len, int64_t* d_input_ids,
                                   int64_t* d_token_type_ids, int64_t* d_attention_mask,
                                   int64_t* d_labels, int64_t* d_next_sentence_labels,
                                   float mlm_probability, int64_t ignore_index, int64_t vocab_len,
                                   uint64_t seed, uint64_t counter,
                                   const lddl_span_params* params);

int lddl_collate_pairs_seqpack_masked_span(
    lddl_ctx* ctx, void* stream, const void* d_tokens, const int64_t* d_tok_off,
    const int32_t* d_len_a, const uint8_t* d_is_rn, const int64_t* d_rows, int32_t batch,
    const int64_t* d_dst, const int32_t* d_fill, const int32_t* d_seq_in_row,
    const int32_t* d_packed_idx, int32_t out_rows, int32_t max_seq_length, int32_t draw_stride,
    int64_t* d_input_ids, int64_t* d_token_type_ids, int64_t* d_attention_mask, int64_t* d_labels,
    int64_t* d_position_ids, int64_t* d_sequence_ids, int64_t* d_next_sentence_labels,
    int64_t* d_cls_positions, int32_t* d_seq_lens, float mlm_probability, int64_t ignore_index,
    int64_t vocab_len, uint64_t seed, uint64_t counter, const lddl_span_params* params);

/* ---------------------------------------------------------------------------------------------
 * Compact MLM targets from dense labels (past the reference): the masked slots of
 * d_labels int64[R * L] (label != ignore_index) in position order as fixed-shape arrays, for a
 * gather in front of the MLM head. Asynchronous on `stream`; no context, no temporaries, no
 * host wait, safe in a captured step. Every element of every output is written exactly once
 * per call (the outputs need no initialisation).
 *
 * lddl_mlm_compact_rows: row r's masked slots x_0 < x_1 < ..., n_r of them, k = min(n_r, P):
 *   d_positions[r * P + j] = x_j, d_ids[r * P + j] = labels[r, x_j], d_weights[r * P + j] = 1
 *   for j < k; 0, ignore_index and 0 for k <= j < P; d_num_masked[r] = n_r, the true count, so
 *   n_r > P tells an overflow (the first P slots in position order are the ones kept).
 * lddl_mlm_compact_flat: the same over labels.view(-1): the flat indices r * L + x ascending in
 *   d_flat_positions[capacity] with their labels in d_flat_ids[capacity]; the first
 *   min(total, capacity) are kept, the rest is position 0 and id ignore_index;
 *   d_num_masked[r] = n_r and *d_total (device int64) = sum of n_r.
 *
 * Both fail with -1 before anything is launched on a NULL pointer, R < 0, L < 0, L > 2^31 - 1
 * (the counts are int32), or P < 1 / capacity < 1. R == 0 launches nothing for the rows form;
 * the flat form then still writes its padding and *d_total = 0. L == 0 is R rows without a
 * masked slot: all padding, counts 0.
 * ------------------------------------------------------------------------------------------- */
int lddl_mlm_compact_rows(void* stream, const int64_t* d_labels, int64_t R, int64_t L,
                          int64_t ignore_index, int64_t P, int64_t* d_positions, int64_t* d_ids,
                          float* d_weights, int32_t* d_num_masked);
int lddl_mlm_compact_flat(void* stream, const int64_t* d_labels, int64_t R, int64_t L,
                          int64_t ignore_index, int64_t capacity, int64_t* d_flat_positions,
                          int64_t* d_flat_ids, int32_t* d_num_masked, int64_t* d_total);

/* ---------------------------------------------------------------------------------------------
 * BART denoising (past the reference): sentence permutation and text infilling of
 * tokenized documents, one launch per batch, asynchronous on `stream`, no temporaries, no host
 * wait. The input is lddl_tokenize's output read in place: sentence s holds
 * d_sent_len[s] & (2^30 - 1) pieces from d_ids[d_sent_off[s]]; document (= sample) d holds the
 * sentences d_doc_sent_off[d] .. d_doc_sent_off[d + 1]; output row i is sample d_rows[i], or i
 * with d_rows NULL. int64 [batch, seq_len] d_input_ids, d_attention_mask, d_decoder_input_ids
 * and d_labels and int32 [batch] d_src_lengths are written in full. L = seq_len, per row i:
 *   budget   the sample keeps its first T = L - 2 pieces in original order: the sentence that
 *     crosses T is cut and the sentences after it have length 0;
 *   units    sentence u < LDDL_DENOISE_MAX_UNITS - 1 is unit u; the sentences from
 *     LDDL_DENOISE_MAX_UNITS - 1 on are one tail unit and keep their order inside it;
 *   sentence permutation   rs(u) = Philox4x32-10 at flat index i * draw_stride + u (the
 *     collates' counter layout: flat low, flat high, counter low, counter high) under the key
 *     seed ^ LDDL_DENOISE_SENT_XOR; a unit of non-zero length takes part iff
 *     u01(rs(u).x) < permute_p (u01(v) = (v >> 8) * 2^-24); the participants sorted by
 *     (rs(u).y, u) fill the participants' places in order, every other unit stays;
 *   words    over the permuted sequence, slot x is a head iff it is the first piece of a
 *     sentence or its id is no continuation ("##x") id; word(x) = the heads at or before x, - 1;
 *   spans    r(x) = the same Philox call at flat index i * draw_stride + x under the key seed; a
 *     head of word j starts a span iff u01(r.x) < p_start; its length is
 *     len = #{k in [0, n) : u01(r2.x) >= cum[k]}, r2 the call at the same index under the key
 *     seed ^ LDDL_SPAN_SEED_XOR; e(j) = j + len for a starting word, else 0; E(j) = the maximum
 *     of e over the words before j;
 *   emission   a slot of word j: nothing if E(j) > j (the run already has its noise token);
 *     else, if the word starts a span of len >= 1, its head gives one noise token and its
 *     continuations nothing; else, if it starts one of len = 0, its head gives a noise token
 *     and then its id, its continuations their ids; else its id. The noise token is
 *     (r.w * vocab_len) >> 32 if u01(r.y) < random_ratio, else mask_id;
 *   rows     input_ids = bos, the emitted ids, eos, then pad; src_lengths = the emitted count
 *     + 2, untruncated: beyond L the ids at destinations >= L - 1 are dropped and eos sits at
 *     L - 1; attention_mask = 1 up to and including eos; labels = bos, the budgeted pieces in
 *     original order, eos, then ignore_index; decoder_input_ids = decoder_start_id, then labels
 *     one slot to the right, pad where that label is ignored.
 * permute_p = 0 is the identity; p_start = 0 leaves the permuted sample.
 *
 * lddl_denoise_params_make (host only): P(len = k) proportional to weights[k], k = 0 .. n (n + 1
 * entries; NULL: Poisson(3) on 0 .. n, the default being n = 10); cum[k] = float(P(len <= k))
 * for k < n and 1 from there on; p_start solves 1 - prod_{k < n} (1 - s * P(len > k)) =
 * mask_ratio, the probability that a word deep in a row is deleted or replaced (inserted noise
 * tokens do not count), by lddl_span_params_make's bisection. Fails with -1 on n outside
 * [1, LDDL_SPAN_MAX_N], a negative, non-finite or all-zero weight list, mask_ratio outside
 * [0, 1] or above what p_start = 1 reaches, or out NULL.
 *
 * lddl_bart_denoise fails with -1 before anything is launched on a NULL ctx, params NULL or not
 * such as lddl_denoise_params_make writes (n, p_start in [0, 1], cum rising within [0, 1] below
 * n and 1 from n on), seq_len < 2 or > 2^24, draw_stride < seq_len, permute_p or random_ratio
 * outside [0, 1], vocab_len outside [1, 2^32], and, with batch > 0, a NULL table or output.
 * batch <= 0 returns 0 and launches nothing. The row indices are the caller's to check.
 * ------------------------------------------------------------------------------------------- */
#define LDDL_DENOISE_MAX_UNITS 256
#define LDDL_DENOISE_SENT_XOR 0xD1B54A32D192ED03ull
typedef struct {
  int32_t n;                   /* longest span, in words */
  float p_start;               /* a head starts a span with this probability */
  float cum[LDDL_SPAN_MAX_N];  /* cum[k] = P(len <= k) for k < n, 1 from there on */
} lddl_denoise_params;

int lddl_denoise_params_make(double mask_ratio, int32_t n, const double* weights,
                             lddl_denoise_params* out);

int lddl_bart_denoise(lddl_ctx* ctx, void* stream, const int32_t* d_ids,
                      const int64_t* d_sent_off, const int32_t* d_sent_len,
                      const int64_t* d_doc_sent_off, const int64_t* d_rows, int32_t batch,
                      int32_t seq_len, int64_t* d_input_ids, int64_t* d_attention_mask,
                      int64_t* d_decoder_input_ids, int64_t* d_labels, int32_t* d_src_lengths,
                      int64_t bos_id, int64_t eos_id, int64_t pad_id, int64_t mask_id,
                      int64_t decoder_start_id, int64_t ignore_index, int64_t vocab_len,
                      uint64_t seed, uint64_t counter, int32_t draw_stride, float permute_p,
                      float random_ratio, const lddl_denoise_params* params);
/* The same launch with the continuation bitmap handed in (bit id of word id >> 5 set: id
 * continues a word; ids outside [0, n_ids) never do) in place of the context that owns one:
 * lddl_bpe_cont_bits for a byte-level BPE vocabulary. Refuses what lddl_bart_denoise refuses,
 * with a NULL bitmap or n_ids outside [1, 2^31) where that one refuses a NULL ctx. */
int lddl_bart_denoise_bits(const uint32_t* d_cont_bits, int64_t n_ids, void* stream,
                           const int32_t* d_ids, const int64_t* d_sent_off,
                           const int32_t* d_sent_len, const int64_t* d_doc_sent_off,
                           const int64_t* d_rows, int32_t batch, int32_t seq_len,
                           int64_t* d_input_ids, int64_t* d_attention_mask,
                           int64_t* d_decoder_input_ids, int64_t* d_labels,
                           int32_t* d_src_lengths, int64_t bos_id, int64_t eos_id,
                           int64_t pad_id, int64_t mask_id, int64_t decoder_start_id,
                           int64_t ignore_index, int64_t vocab_len, uint64_t seed,
                           uint64_t counter, int32_t draw_stride, float permute_p,
                           float random_ratio, const lddl_denoise_params* params);

/* ---------------------------------------------------------------------------------------------
 * Byte-level BPE (GPT-2 / RoBERTa / BART vocabularies; past the reference).
 * Semantics: GPT-2's encoder.py. Input as lddl_segment_fill lays it out: d_text[n_bytes],
 * d_sent_off[n_sent + 1] rising from 0 to n_bytes (white space between two sentences belongs to
 * the left one), d_doc_sent_off[n_doc + 1] (NULL: every sentence is a document of its own).
 *
 * Pre-tokens. Per document (the match restarts at a document's first byte and sees nothing
 * outside the document) the text is cut by
 *   's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+
 * with \p{L} = general category L*, \p{N} = N*, \s = the White_Space property (U+0009-000D,
 * 0020, 0085, 00A0, 1680, 2000-200A, 2028, 2029, 202F, 205F, 3000; U+001C-001F are not in it)
 * and every other character "other", combining marks included. A byte that is no part of a
 * whole sequence (a lead byte C2-F4 with its 1 to 3 continuation bytes inside the document) is
 * a character of class "other" by itself. The pattern partitions the text. Stated as a local
 * rule (csrc/bpe_split.hip): a white-space character starts a pre-token iff no white space
 * stands before it or a non-space follows it; a non-space starts one after nothing and after
 * white space other than U+0020, never after U+0020, never inside a contraction that fired,
 * always right after one, and otherwise iff its class differs from the class before; a
 * contraction fires at an apostrophe with a letter, a number, white space other than U+0020
 * or nothing before it.
 * Merges. A pre-token starts as the base tokens of its bytes. Repeat: of the adjacent pairs
 * take the one of lowest rank and replace all its occurrences, left to right without overlap,
 * by the merged token; stop when no adjacent pair has a rank.
 * The one deviation: a pre-token longer than LDDL_BPE_MAX_WORD bytes is merged in consecutive
 * slices of LDDL_BPE_MAX_WORD bytes from its first byte (WordPiece's 100-character rule has the
 * same place). Every pre-token up to that length is exact.
 * Assignment. A pre-token belongs to the sentence that holds its LAST byte, so the pieces of a
 * document's sentences, concatenated, are encode(document): " World" after "Hello. " goes to
 * the second sentence.
 * Output, lddl_tokenize's layout: sentence s has its pieces at d_ids[d_sent_off[s] ..] and
 * d_sent_len[s] = min(pieces, max_pieces, bytes of the sentence): the first ones are kept, and
 * no flag bit is set. The bytes of the sentence bound it because its slots do: a sentence that
 * takes over the white space before it can hold one piece more than it has bytes when hardly
 * anything in it merges (sentence "a" after "a ": the pieces " ", "a" in one slot). With a
 * vocabulary that merges a space into the word after it, this does not come up.
 *
 * lddl_bpe_create: class_table = the two-level table that lddl_amd.bpe.load_classes packs
 * from lddl_amd/assets/bpe_classes.txt (tools/bpe_classes.py; a 32-byte header with the Unicode
 * version, 4352 uint16 page indices, 64-byte pages of 2-bit classes); token
 * i is token_bytes[token_off[i] .. token_off[i + 1]) (raw bytes: JSON and GPT-2's byte-to-
 * unicode map are undone by the caller); merges[n_merges][3] = {left, right, merged} ids in
 * rank order. Fails with -1 (lddl_last_error) on a malformed class table, a byte value without
 * a single-byte token, an id outside the vocabulary, an operand that is neither a single-byte
 * token nor the result of an earlier line, a `merged` whose bytes are not left + right, a pair
 * that an earlier line has, or 2^26 merges and more. Builds on `device`: the pair table (open
 * addressing, at most half full), the byte -> id map, the class table, and the continuation
 * bitmap of lddl_bpe_cont_bits: bit id set iff token id can be reached from bytes (a single-
 * byte token or a merge result) and its bytes do not start with 0x20 (fairseq's
 * is_beginning_of_word, negated; special tokens count as beginnings). The pointers of
 * lddl_bpe_cont_bits live as long as the lddl_bpe.
 * lddl_bpe_info: unicode_version[3] of the class table; any pointer may be NULL.
 * lddl_bpe_tokenize: asynchronous on `stream`, no host wait; its temporaries (about 5.5 bytes
 * per byte of text) come from an arena the lddl_bpe owns and are reused by the next call.
 * Fails with -1 on a NULL lddl_bpe, a negative size, max_pieces < 1, or, with n_sent > 0, a
 * NULL array; n_sent = 0 launches nothing.
 *
 * The cl100k pattern (Llama 3, GPT-4, Qwen2 / 2.5, DeepSeek).
 * lddl_bpe_set_pattern(bpe, "cl100k", digit_group) makes lddl_bpe_tokenize and
 * lddl_bpe_pretoken_stats cut a document by
 *   (?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+
 * with digit_group 3, and with \p{N} in place of \p{N}{1,3} (Qwen2) with digit_group 1: what
 * Python's `regex.findall` returns. Documents, classes, \s and ill-formed bytes as above; the
 * contraction letters match ASCII in either case, and U+017F (long s) counts as s. Stated as
 * rules (csrc/bpe_split_cl.hip):
 *   digit       the k-th character (from 0) of a maximal run of digits starts a pre-token iff
 *               k % digit_group == 0; nothing absorbs a run's first digit.
 *   other       starts iff the character before is neither "other" nor U+0020 (the U+0020
 *               opened the token). An apostrophe that starts and is followed by a contraction
 *               fires: the contraction is a pre-token and the character behind it starts.
 *   letter      the first letter of a run starts unless the character before absorbs it: a
 *               starting "other" that did not fire ("(b" is one pre-token, "((b" is "((", "b"),
 *               or white space other than \r and \n ("a\xa0b" is "a", "\xa0b").
 *   white space of a maximal run M: the newlines at M's head that directly follow an "other"
 *               belong to that pre-token. The rest W starts at its first character; if W holds
 *               a newline, that pre-token runs to W's last newline. The remainder R starts at
 *               its first character, and if R has two characters or more and a character
 *               follows the run, R's last character starts as well (it goes with a following
 *               letter, with a following "other" if it is U+0020, and is a pre-token by itself
 *               otherwise). At a document's end R is one pre-token.
 * "gpt2" with digit_group 0 restores the default. Fails with -1 on any other pattern or
 * digit_group.
 * lddl_bpe_set_whole_words(bpe, 1): `ignore_merges` of a Hugging Face tokenizer.json (Llama 3
 * sets it). After the split, a pre-token of 2 to LDDL_BPE_MAX_WORD bytes whose bytes equal a
 * vocabulary entry is that one id (the lowest of equal entries); for every other pre-token the
 * merges decide. 0 restores the default; any other value fails with -1.
 * Both settings hold for the calls issued after them; the temporaries of the cl100k split are
 * 3 bytes per 64 bytes of text more. lddl_bpe_create builds the whole-word table for every
 * lddl_bpe, set or not: 16 bytes per slot (a power of two, at least twice the tokens of 2 bytes
 * and more), a copy of token_bytes and of token_off on the device; about 6 MB for a vocabulary
 * of 128k tokens.
 * ------------------------------------------------------------------------------------------- */
#define LDDL_BPE_MAX_WORD 1024
typedef struct lddl_bpe lddl_bpe;
int lddl_bpe_create(int device, const uint8_t* class_table, int64_t class_len,
                    const uint8_t* token_bytes, const int64_t* token_off, int64_t n_tokens,
                    const int32_t* merges, int64_t n_merges, lddl_bpe** out);
int lddl_bpe_destroy(lddl_bpe* bpe);
int lddl_bpe_info(const lddl_bpe* bpe, int64_t* n_tokens, int64_t* n_merges,
                  int32_t* unicode_version, int32_t* max_word);
int lddl_bpe_cont_bits(const lddl_bpe* bpe, const uint32_t** d_bits, int64_t* n_ids);
int lddl_bpe_set_pattern(lddl_bpe* bpe, const char* pattern, int32_t digit_group);
int lddl_bpe_set_whole_words(lddl_bpe* bpe, int32_t on);
int lddl_bpe_tokenize(lddl_bpe* bpe, void* stream, const uint8_t* d_text, int64_t n_bytes,
                      const int64_t* d_sent_off, int64_t n_sent, const int64_t* d_doc_sent_off,
                      int64_t n_doc, int32_t max_pieces, int32_t* d_ids, int32_t* d_sent_len);
/* Measurement aid: the pre-tokenizer alone on the same input, asynchronous on `stream`.
 * d_stats (device int64[3]) = the pre-tokens of the text, those of at most 64 bytes that cross
 * the end of the 64-byte tile they start in, and those longer than 64 bytes: the words that
 * csrc/bpe_merge.hip serves in its tile pass's second window and in its long pass. */
int lddl_bpe_pretoken_stats(lddl_bpe* bpe, void* stream, const uint8_t* d_text, int64_t n_bytes,
                            const int64_t* d_sent_off, int64_t n_sent,
                            const int64_t* d_doc_sent_off, int64_t n_doc, int64_t* d_stats);

/* ---------------------------------------------------------------------------------------------
 * SentencePiece unigram (T5 / mT5 / ALBERT / XLNet / XLM-R / mBART vocabularies; past the
 * reference). Input and output are lddl_bpe_tokenize's: d_text[n_bytes],
 * d_sent_off[n_sent + 1] rising from 0 to n_bytes, d_doc_sent_off accepted and unread (a document
 * starts where a sentence does, and a word never crosses a sentence start); sentence s has its
 * pieces at d_ids[d_sent_off[s] ..] and d_sent_len[s] = min(pieces, max_pieces, bytes of s): the
 * first ones are kept and no flag bit is set. The bytes bound it because the slots do ("a b c"
 * on a vocabulary without "▁a" has six pieces in five bytes).
 *
 * Words. A space is the byte 0x20; with LDDL_UNIGRAM_ASCII_WS in `flags` the bytes 0x09, 0x0A,
 * 0x0C and 0x0D are spaces too. A word is a maximal run of non-space bytes inside one sentence,
 * and it is encoded alone as the bytes E2 96 81 (U+2581, the space mark) followed by its own:
 * SentencePiece with add_dummy_prefix, remove_extra_whitespaces, escape_whitespaces and
 * split_by_whitespace at their defaults. That is exact because lddl_unigram_create refuses a
 * vocabulary with the mark at a non-leading position of a piece, so that the lattice of a
 * sentence falls apart at every word. A sentence without a word has no pieces.
 * Characters. A lead byte C2-DF, E0-EF, F0-F4 with its 1, 2, 3 continuation bytes (80-BF) inside
 * the word is one character; every other byte (a stray continuation byte, the lead of a
 * truncated sequence, C0, C1, F5-FF) is a character of length 1.
 * Viterbi per word of n bytes, mark included: best[0] = 0.0f. For each character start s in
 * rising order and every NORMAL or USER_DEFINED piece that equals bytes[s:e], cand = best[s] +
 * score as one float32 add; cand replaces best[e] iff best[e] is unset or cand > best[e] (strict:
 * the earlier start wins a tie). If no piece of exactly one character matched at s, that
 * character is a candidate too, with id unk_id and score unk_score = (the lowest NORMAL score) -
 * 10.0f. The path is read back from best[n]; consecutive unk_id pieces fuse into one. There is
 * no other floating point. The score of a USER_DEFINED piece is read as given (lddl_amd.unigram
 * passes SentencePiece's length * max score - 0.1 for them).
 * Deviations. This call applies no normaliser beyond the space classes and tokenizes the text
 * it is given (lddl_unigram_normalize_plan / _write below apply the model's rules first);
 * CONTROL, UNKNOWN, UNUSED and BYTE pieces never match text (byte fallback, below, rewrites the
 * finished path). A word of more than LDDL_UNIGRAM_MAX_WORD
 * bytes is encoded in consecutive slices of at most that many of its bytes, each cut at the
 * last character start that fits, each with a Viterbi and an unknown fusion of its own; only
 * the first slice carries the mark.
 *
 * lddl_unigram_create: piece i is piece_bytes[piece_off[i] .. piece_off[i + 1]) with scores[i]
 * and types[i] (1 NORMAL, 2 UNKNOWN, 3 CONTROL, 4 USER_DEFINED, 5 UNUSED, 6 BYTE, as in
 * sentencepiece_model.proto); flags = 0 or LDDL_UNIGRAM_ASCII_WS. Fails with -1
 * (lddl_last_error) on a NULL array, n_pieces outside [1, 2^20], no NORMAL or USER_DEFINED
 * piece that is the mark alone, the mark at an interior position of such a piece, unk_id out of
 * range or not the one UNKNOWN piece, an empty or repeated such piece, a score that is not
 * finite or beyond 1e30 in magnitude (the sums of a slice stay finite), and more than
 * LDDL_UNIGRAM_MAX_NEST pieces on one root-to-leaf path of the byte trie: that is the most
 * matches one start can have, and max_sentencepiece_length = 16, the default, keeps a model
 * inside it. Builds on `device`: the trie as an open-addressing table (node, byte) -> (child,
 * piece or -1, score) of 16-byte slots, at most half full, a 256-entry table for the root, and
 * the bitmap of lddl_unigram_cont_bits: bit id set iff piece id is NORMAL or USER_DEFINED and
 * does not start with the mark (the shape of lddl_bpe_cont_bits; an unknown piece counts as a
 * word's beginning). Its pointers live as long as the lddl_unigram.
 * lddl_unigram_info: the pieces, the trie's nodes, the bytes of the two tables, unk_score; any
 * pointer may be NULL.
 * lddl_unigram_tokenize: asynchronous on `stream`, no host wait; its temporaries (about 5 bytes
 * per byte of text) come from an arena the lddl_unigram owns and are reused by the next call.
 * Fails with -1 on a NULL lddl_unigram, a negative size, max_pieces < 1, or, with n_sent > 0, a
 * NULL array; n_sent = 0 launches nothing.
 * lddl_unigram_word_stats: measurement aid, the word marks alone on the same input. d_stats
 * (device int64[3]) = the words, those of at most 64 bytes that cross the end of the 64-byte
 * tile they start in (the tile pass's second window) and those longer than 64 bytes (the long
 * pass of csrc/unigram_viterbi.hip).
 * ------------------------------------------------------------------------------------------- */
#define LDDL_UNIGRAM_MAX_WORD 1024
#define LDDL_UNIGRAM_MAX_NEST 16
#define LDDL_UNIGRAM_ASCII_WS 1
typedef struct lddl_unigram lddl_unigram;
int lddl_unigram_create(int device, const uint8_t* piece_bytes, const int64_t* piece_off,
                        const float* scores, const int32_t* types, int64_t n_pieces,
                        int32_t unk_id, int32_t flags, lddl_unigram** out);
int lddl_unigram_destroy(lddl_unigram* unigram);
int lddl_unigram_info(const lddl_unigram* unigram, int64_t* n_pieces, int64_t* n_nodes,
                      int64_t* table_bytes, float* unk_score, int32_t* max_word);
int lddl_unigram_cont_bits(const lddl_unigram* unigram, const uint32_t** d_bits, int64_t* n_ids);
int lddl_unigram_tokenize(lddl_unigram* unigram, void* stream, const uint8_t* d_text,
                          int64_t n_bytes, const int64_t* d_sent_off, int64_t n_sent,
                          const int64_t* d_doc_sent_off, int64_t n_doc, int32_t max_pieces,
                          int32_t* d_ids, int32_t* d_sent_len);
int lddl_unigram_word_stats(lddl_unigram* unigram, void* stream, const uint8_t* d_text,
                            int64_t n_bytes, const int64_t* d_sent_off, int64_t n_sent,
                            const int64_t* d_doc_sent_off, int64_t n_doc, int64_t* d_stats);

/* ---------------------------------------------------------------------------------------------
 * SentencePiece unigram: the model's normaliser and byte fallback. Both are off on
 * a new lddl_unigram, which then behaves as stated above, bit for bit.
 *
 * Normaliser. A rule is (key, replacement), two byte strings; the rules are the enumerated
 * precompiled_charsmap of the model (lddl_amd.unigram.load_normalizer). The pass follows
 * SentencePiece's Normalizer::Normalize at add_dummy_prefix = remove_extra_whitespaces =
 * escape_whitespaces = true. Per sentence, left to right from its first byte, at position i:
 *   - the longest key that equals the bytes at i and ends inside the sentence: its replacement
 *     (it may be empty) is emitted and i advances by the key's length;
 *   - else, if a well-formed UTF-8 character starts at i and ends inside the sentence (no
 *     overlong form, no surrogate, at most U+10FFFF), it is emitted unchanged and i advances by
 *     its length;
 *   - else EF BF BD (U+FFFD) is emitted and i advances by one byte.
 * The scan is greedy and sequential: a position inside a consumed key is never a start, and no
 * match crosses a sentence's end. Spaces in the output are not collapsed, stripped or escaped
 * here: lddl_unigram_tokenize splits on runs of spaces and prefixes every word with the mark,
 * so a replacement by a space, or by nothing, needs no more. While a normaliser is set,
 * LDDL_UNIGRAM_ASCII_WS is ignored by lddl_unigram_tokenize and lddl_unigram_word_stats: the
 * rules decide what becomes a space. Stated departure: a replacement with two interior spaces
 * gives SentencePiece a piece that is the mark alone; here the spaces collapse.
 * lddl_unigram_set_normalizer: rule r is key_blob[key_off[r] .. key_off[r + 1]) ->
 * repl_blob[repl_off[r] .. repl_off[r + 1]), host arrays; n_rules = 0 turns the normaliser off
 * (the arrays are unread). Fails with -1 on a NULL array, an empty key, a key of more than
 * LDDL_UNIGRAM_NORM_MAX_KEY bytes (a key spans two 64-byte tiles at most, and up to that length
 * no key makes a tile of plain text wait for the tile before it), a repeated key, more
 * than 2^24 rules or offsets that do not rise from 0. It builds a byte trie of the keys in the
 * layout of the pieces' trie, a (offset, length) pair per rule, the replacement blob and the
 * masks of the bytes and byte pairs that start a key. It waits for the device (a set-up call).
 * lddl_unigram_normalize_plan: asynchronous on `stream`, no host wait. Writes
 * d_out_sent_off[n_sent + 1] (int64), the sentence offsets of the normalised text; the last
 * entry is its size. d_sent_off rises from 0 to n_bytes. The plan's per-tile temporaries (17
 * bytes per 64 of text, from the lddl_unigram's arena) stay until the next plan.
 * lddl_unigram_normalize_write: asynchronous, no host wait; must follow the plan of the same
 * d_text, n_bytes, d_sent_off and n_sent on the same lddl_unigram and the same stream (-1
 * otherwise: the plan's temporaries return to the arena on the plan's stream), with
 * d_out_sent_off as the plan wrote it, and writes the normalised text to d_out_text[out_cap].
 * Fails with -1 and a message if out_cap is below the planned size, which it knows without
 * waiting once the caller has waited for the plan (as a caller that sized d_out_text by
 * d_out_sent_off[n_sent] has); in any case no byte is stored at or past out_cap.
 *
 * Byte fallback. lddl_unigram_set_byte_pieces(ids256): ids256[b] is the piece of byte b (the
 * BYTE pieces <0x00> .. <0xFF> of the model), a host array; NULL turns it off. -1 on an id
 * outside the vocabulary. It runs after the Viterbi, which is unchanged and still scores an
 * unknown character at unk_score: every unk_id piece of the finished path is replaced by one
 * piece per byte of the fused run of unknown characters it stands for, ids256[byte] in byte
 * order. Pieces per byte stay at most 1, so the d_ids layout and d_sent_len's bounds hold. The
 * bitmap of lddl_unigram_cont_bits gets the bits of the 256 ids: a byte piece always follows
 * the mark or another piece of its word, which holds because lddl_unigram_create requires the
 * mark to be a piece of its own, so that an unknown character never opens a word's pieces.
 * lddl_unigram_cont_bits_host copies that bitmap, (n_pieces + 31) / 32 words, to the host
 * (it waits for the copy).
 * lddl_unigram_normalize_stats: measurement aid on the plan's stream; d_stats (device int64[2])
 * = the tiles of the last plan and those that take the dirty path.
 * lddl_unigram_norm_info: the rules, the longest key and replacement in bytes, whether byte
 * fallback is on; any pointer may be NULL.
 * ------------------------------------------------------------------------------------------- */
#define LDDL_UNIGRAM_NORM_MAX_KEY 61
int lddl_unigram_set_normalizer(lddl_unigram* unigram, const uint8_t* key_blob, const int64_t* key_off,
                                const uint8_t* repl_blob, const int64_t* repl_off, int64_t n_rules);
int lddl_unigram_set_byte_pieces(lddl_unigram* unigram, const int32_t* ids256);
int lddl_unigram_norm_info(const lddl_unigram* unigram, int64_t* n_rules, int32_t* max_key,
                           int32_t* max_repl, int32_t* byte_fallback);
int lddl_unigram_normalize_plan(lddl_unigram* unigram, void* stream, const uint8_t* d_text,
                                int64_t n_bytes, const int64_t* d_sent_off, int64_t n_sent,
                                int64_t* d_out_sent_off);
int lddl_unigram_normalize_stats(lddl_unigram* unigram, void* stream, int64_t* d_stats);
int lddl_unigram_cont_bits_host(const lddl_unigram* unigram, uint32_t* bits);
int lddl_unigram_normalize_write(lddl_unigram* unigram, void* stream, const uint8_t* d_text,
                                 int64_t n_bytes, const int64_t* d_sent_off, int64_t n_sent,
                                 const int64_t* d_out_sent_off, uint8_t* d_out_text, int64_t out_cap);

/* ---------------------------------------------------------------------------------------------
 * RoBERTa blocks (past the reference): rows of contiguous whole sentences without
 * NSP, cut over a whole round of sentences and collated with dynamic masking. FULL-SENTENCES
 * and DOC-SENTENCES of the RoBERTa paper; fairseq's TokenBlockDataset(break_mode='complete' /
 * 'complete_doc') with MaskTokensDataset. The input is a token table as lddl_tokenize and
 * lddl_bpe_tokenize lay it out: d_ids, d_sent_off[n_sent + 1], d_sent_len[n_sent] (its flag
 * bits above bit 29 are masked off: len(s) = d_sent_len[s] & (2^30 - 1)) and
 * d_doc_sent_off[n_doc + 1]. T = seq_len - 2 >= 1.
 *   cost    sep(s) = 1 in LDDL_BLOCKS_FULL if s is the last sentence of non-zero length of its
 *     document, else 0; always 0 in LDDL_BLOCKS_DOC. c(s) = min(len(s) + sep(s), T); the
 *     sentence keeps its first c(s) - sep(s) pieces; an empty sentence costs 0. The separator
 *     belongs to the end of its document, so a sentence's cost does not depend on where its
 *     block starts. This is the one deviation from fairseq, where the blank line between two
 *     documents is an item of its own and may open a block.
 *   jump    P = the exclusive prefix sum of c in int64 (P[n_sent] the total); next(i) = the
 *     largest j > i with P[j] - P[i] <= T (next(i) >= i + 1 because c <= T); in LDDL_BLOCKS_DOC
 *     next(i) is at most the end of i's document, the first entry of d_doc_sent_off above i.
 *   blocks  b_0 = 0, b_{k + 1} = next(b_k) until n_sent is reached; block k is the sentences
 *     [b_k, b_{k + 1}) and its length P[b_{k + 1}] - P[b_k]. A block of length 0 is not emitted
 *     (a document of empty sentences only in DOC mode; an input of empty sentences only).
 *
 * lddl_blocks_plan writes d_piece_off[n_sent + 1] = P, d_sent_sep[n_sent] = sep, the emitted
 * blocks in order as d_block_sent[k] = b_k and d_block_len[k], d_block_sent[n_blocks] = n_sent
 * and d_n_blocks[0]; d_block_sent and d_block_len have room for n_sent + 1 entries. Block k ends
 * at d_block_sent[k + 1] wherever the next emitted block starts: the sentences between are
 * empty. Asynchronous on `stream`, no host wait (the caller reads d_n_blocks once per round);
 * the temporaries, 17 bytes a sentence, come from an arena that the library keeps per device
 * and lddl_blocks_release() empties (it waits for the work that used them). Fails with -1
 * before anything is launched on seq_len < 3 or > 2^24, a mode that is neither, a negative
 * size, a NULL output, or, with n_sent > 0, a NULL input. n_sent = 0 gives n_blocks = 0.
 * The walk is on two levels, tiles of LDDL_BLOCKS_TILE sentences (csrc/blocks_plan.hip).
 *
 * lddl_collate_blocks / lddl_collate_blocks_masked: output row i is block d_rows[i] (d_rows
 * NULL: block i; the indices are the caller's to check) of the plan made with the same seq_len:
 *   input_ids = bos_id, the kept pieces of the block's sentences in order with eos_id behind a
 *     sentence that has sep = 1, eos_id, then pad_id; attention_mask = 1 up to and including
 *     the closing eos_id.
 *   specials   bos, every eos (separators included) and pad are special: never masked, no
 *     word, and a span runs on over them as in the n-gram entry points above.
 *   masking    slot x of row i draws r = the Philox call of lddl_mask_dynamic at flat index
 *     i * seq_len + x under seed and counter. params NULL: per token, masked iff not special
 *     and u01(r.x) < mlm_probability. params given (word mode): a slot is a head iff it is not
 *     special and it is the first kept piece of a sentence or its id is no continuation id
 *     (bit id of d_cont_bits[id >> 5]; ids outside [0, n_ids) never continue a word:
 *     lddl_bpe_cont_bits, or a WordPiece "##" bitmap); words, starts (params->p_start), lengths
 *     and the prefix maximum are those of the n-gram entry points, mlm_probability is unread,
 *     and n = 1 is whole-word masking. Both modes: 80 / 10 / 10 with mask_id and the random id
 *     (r.w * vocab_len) >> 32, labels = the id where masked, else ignore_index.
 *   unmasked   d_special_tokens_mask (1 on special slots) is written in place of labels.
 * All outputs are int64 [batch, seq_len], every element written exactly once. One launch,
 * asynchronous, no temporaries. A block of more than LDDL_BLOCKS_LDS_SENTS sentences is served
 * from global memory past that many. Both fail with -1 before anything is launched on
 * seq_len < 3 or > 2^24 and, with batch > 0, a NULL table, plan or output; the masked one also
 * on params that lddl_span_params_make cannot have written, mlm_probability outside [0, 1],
 * vocab_len outside [1, 2^32], n_ids outside [1, 2^31), and params with a NULL bitmap.
 * batch <= 0 returns 0 and launches nothing.
 * ------------------------------------------------------------------------------------------- */
#define LDDL_BLOCKS_FULL 0
#define LDDL_BLOCKS_DOC 1
#define LDDL_BLOCKS_TILE 2048
#define LDDL_BLOCKS_LDS_SENTS 256
int lddl_blocks_plan(void* stream, const int32_t* d_sent_len, int64_t n_sent,
                     const int64_t* d_doc_sent_off, int64_t n_doc, int32_t seq_len, int32_t mode,
                     int64_t* d_piece_off, uint8_t* d_sent_sep, int64_t* d_block_sent,
                     int32_t* d_block_len, int64_t* d_n_blocks);
int lddl_blocks_release(void);
int lddl_collate_blocks(void* stream, const int32_t* d_ids, const int64_t* d_sent_off,
                        const int64_t* d_piece_off, const uint8_t* d_sent_sep,
                        const int64_t* d_block_sent, const int64_t* d_rows, int32_t batch,
                        int32_t seq_len, int64_t* d_input_ids, int64_t* d_attention_mask,
                        int64_t* d_special_tokens_mask, int64_t bos_id, int64_t eos_id,
                        int64_t pad_id);
int lddl_collate_blocks_masked(const uint32_t* d_cont_bits, int64_t n_ids, void* stream,
                               const int32_t* d_ids, const int64_t* d_sent_off,
                               const int64_t* d_piece_off, const uint8_t* d_sent_sep,
                               const int64_t* d_block_sent, const int64_t* d_rows, int32_t batch,
                               int32_t seq_len, int64_t* d_input_ids, int64_t* d_attention_mask,
                               int64_t* d_labels, int64_t bos_id, int64_t eos_id, int64_t pad_id,
                               int64_t mask_id, float mlm_probability, int64_t ignore_index,
                               int64_t vocab_len, uint64_t seed, uint64_t counter,
                               const lddl_span_params* params);

/* ---------------------------------------------------------------------------------------------
 * T5 span corruption (past the reference): an exact number of noise tokens in an
 * exact number of spans per row, written as two compacted rows with matching sentinel ids. T5's
 * random_spans_noise_mask with noise_span_to_unique_sentinel; the two stated deviations are the
 * fixed-point counts and the RNG. Row i is block d_rows[i] (NULL: block i; the indices are the
 * caller's to check) of a lddl_blocks_plan plan made with plan_seq_len, FULL or DOC. Its tokens
 * t[0 .. n) are the block's kept pieces in order with eos_id where the plan put a separator
 * (an ordinary token here); n = P[b_{k + 1}] - P[b_k] <= T = plan_seq_len - 2. No bos.
 *   counts  in int64, no floating point: dq = round(noise_density * 65536) and iq = round(65536
 *     / mean_noise_span_length) are the caller's, made once.
 *     N = clamp((n * dq + 32768) >> 16, 1, n - 1) noise tokens,
 *     k = clamp((N * iq + 32768) >> 16, 1, min(N, n - N, n_sentinels)) spans, M = n - N;
 *     n < 2: N = k = 0 (the row is its tokens and eos, the target eos alone).
 *   keys    for u in [0, max(N, M) - 1), r(u) = the Philox call of lddl_mask_dynamic at flat
 *     index i * plan_seq_len + u under seed and counter; noise item u + 1 has the key r.x >> 8,
 *     non-noise item u + 1 the key r.y >> 8 (24 bits).
 *   segments  of the noise items 1 .. N - 1 the k - 1 with the smallest (key, item) pairs in
 *     lexicographic order open a segment, and so does item 0; B[g] = the first item of noise
 *     segment g in ascending order, B[k] = N. The non-noise items 1 .. M - 1 give A[g] in the
 *     same way from their keys, A[k] = M. Every segment holds an item.
 *   order   non-noise segment 0, noise segment 0, non-noise segment 1, ...: the row starts clean
 *     and ends in noise. Noise item j of segment g is t[j + A[g + 1]], non-noise item m of
 *     segment h is t[m + B[h]]. Sentinel g has the id sentinel_first - g.
 *   input_ids [batch, in_len]: for g = 0 .. k - 1 non-noise segment g, then sentinel g; then
 *     eos_id; then pad_id. attention_mask = 1 up to and including that eos_id.
 *   labels [batch, tgt_len]: for g = 0 .. k - 1 sentinel g, then noise segment g; then eos_id;
 *     then ignore_index (no closing sentinel).
 *   decoder_input_ids [batch, tgt_len]: decoder_start_id, then labels shifted right by one with
 *     pad_id in the slots where labels is ignore_index's fill.
 *   src_lengths, tgt_lengths int64 [batch] = M + k + 1 and N + k + 1, never truncated.
 * An id whose slot lies at or past the last slot of a row that is too narrow is dropped, and the
 * eos_id sits in the last slot. Every output element is written exactly once. One launch,
 * asynchronous on `stream`, no temporaries, no atomics on global memory.
 *
 * lddl_t5_lengths (host only): *in_len = M + k + 1 and *tgt_len = N + k + 1 at n = tokens. Both
 * are non-decreasing in n, so no row of a plan with T = tokens overflows them.
 * Both fail with -1 before anything is launched on plan_seq_len < 3 or > 2^24 (tokens < 1 or
 * > 2^24 - 2), in_len or tgt_len outside [1, 2^24], dq outside [1, 65535], iq outside
 * [1, 65536], n_sentinels outside [1, LDDL_T5_MAX_SPANS], sentinel_first - n_sentinels + 1 < 0
 * and, lddl_t5_lengths always and lddl_t5_corrupt with batch > 0, a NULL table, plan or output.
 * batch <= 0 returns 0 and launches nothing.
 * ------------------------------------------------------------------------------------------- */
#define LDDL_T5_MAX_SPANS 256
int lddl_t5_lengths(int64_t tokens, int32_t dq, int32_t iq, int32_t n_sentinels, int64_t* in_len,
                    int64_t* tgt_len);
int lddl_t5_corrupt(void* stream, const int32_t* d_ids, const int64_t* d_sent_off,
                    const int64_t* d_piece_off, const uint8_t* d_sent_sep,
                    const int64_t* d_block_sent, const int64_t* d_rows, int32_t batch,
                    int32_t plan_seq_len, int32_t in_len, int32_t tgt_len, int32_t dq, int32_t iq,
                    int32_t n_sentinels, int64_t sentinel_first, int64_t eos_id, int64_t pad_id,
                    int64_t decoder_start_id, int64_t ignore_index, uint64_t seed,
                    uint64_t counter, int64_t* d_input_ids, int64_t* d_attention_mask,
                    int64_t* d_labels, int64_t* d_decoder_input_ids, int64_t* d_src_lengths,
                    int64_t* d_tgt_lengths);

/* ---------------------------------------------------------------------------------------------
 * The GPT stream (past the reference): rows for causal language modelling, cut from
 * one endless stream doc, eos, doc, eos, ... of the round's documents; Megatron-LM's GPT dataset
 * with reset_position_ids / eod_mask_loss, and the document-level fill-in-the-middle transform
 * of Bavarian et al. 2022 applied before packing. A row starts and ends anywhere inside a
 * document and no slot is padded. The input is a token table as lddl_tokenize and
 * lddl_bpe_tokenize lay it out: d_ids, d_sent_off[n_sent + 1], d_sent_len[n_sent] (len(s) =
 * d_sent_len[s] & (2^30 - 1); gaps between sentences allowed) and d_doc_sent_off[n_doc + 1]. A
 * document's tokens are the concatenated pieces of its sentences, t(d) of them, fewer than
 * 2^31 - 4.
 *   order   d_doc_order, an int64 permutation of [0, n_doc) on the device, or NULL for the
 *     identity: the stream takes document d_doc_order[j] at place j (the caller's to check; an
 *     id outside is clamped).
 *   FIM     per document r = the Philox call of lddl_mask_dynamic at index d, the document's id
 *     in the table (not its place, so the shuffle does not change a document's transform),
 *     under seed and counter. fim_q and spm_q are the two rates in 16.16 fixed point, rounded
 *     half up by the caller, in [0, 65536]. A document with t >= 1 is transformed iff
 *     (r.x >> 16) < fim_q; it takes the SPM layout iff it is transformed and (r.y >> 16) <
 *     spm_q, else PSM. The cuts a <= b are the sorted pair (r.z * (t + 1)) >> 32, (r.w *
 *     (t + 1)) >> 32, both in [0, t]. With prefix = [0, a), middle = [a, b), suffix = [b, t):
 *       PSM  fim_prefix_id prefix fim_suffix_id suffix fim_middle_id middle
 *       SPM  fim_prefix_id fim_suffix_id suffix fim_middle_id prefix middle
 *     Either adds 3 tokens; empty pieces are legal; t = 0 is never transformed. The cuts are
 *     token-level: the stated deviation from the paper's character-level cuts.
 *   stream  cost(d) = t(d) + 1, + 3 when transformed: the + 1 is the terminator eos_id behind
 *     every document, also behind an empty one (a second deviation, from loaders that drop
 *     empty documents), so document offsets rise strictly. Q = the int64 exclusive prefix sum
 *     of cost(d_doc_order[j]) over the places, Q[n_doc] the total. n_rows = max(0, (Q[n_doc] -
 *     1) / L), L = seq_len; row r reads stream positions r * L .. r * L + L, and the tail that
 *     fills no row is dropped.
 *
 * lddl_stream_plan writes d_sent_tok_off[n_sent + 1], the exclusive prefix sum of len(s),
 * d_doc_off[n_doc + 1] = Q, and d_n_rows[0] = n_rows, d_n_rows[1] = Q[n_doc]. Asynchronous on
 * `stream`, no host wait (the caller reads d_n_rows once per plan), no atomics; the scans'
 * scratch comes from an arena that the library keeps per device and lddl_stream_release()
 * empties. No record of the draws is kept: lddl_stream_rows draws them again from the same
 * seed and counter.
 *
 * lddl_stream_rows: output row i is plan row d_rows[i] (NULL: row i; an index outside [0,
 * n_rows) is clamped into it), slot y in [0, L), all int64 [batch, seq_len]:
 *   input_ids[y]    stream token r * L + y.
 *   labels[y]       stream token r * L + y + 1; with eod_mask_loss, ignore_index where the
 *     slot's input is a document's terminator, decided by its position in the stream, not by
 *     comparing ids.
 *   position_ids[y] y minus the slot of the last sequence start at or before y, where the
 *     row's slot 0 is always a start and so is a slot whose predecessor is a terminator;
 *     without reset_position_ids it is y.
 *   sequence_ids[y] the number of terminators in the row's slots before y.
 * There is no attention mask: every slot is real. Every element is written exactly once; one
 * launch, workgroups of LDDL_STREAM_TILE slots, no temporaries, no atomics. A tile that
 * overlaps more than LDDL_STREAM_LDS_DOCS places is served from global memory past that many.
 * The knobs (d_doc_order, fim_q, spm_q, seed, counter) must be the plan's. A plan without a
 * row (or n_doc = 0) writes nothing.
 *
 * lddl_stream_cu_seqlens: d_cu_seqlens int32 [max_seqs + 1] and d_n_seqs int32 [1] for
 * variable-length attention that does not cross documents: the flat offsets i * L + y of every
 * sequence start of the batch in order (slot 0 of each row, every slot y >= 1 whose
 * predecessor is a terminator). cu_seqlens[n_seqs] and everything behind it is batch * L;
 * n_seqs is the untruncated count. If n_seqs > max_seqs, the first max_seqs starts are written
 * and cu_seqlens[max_seqs] = batch * L, so the caller sees the overflow by n_seqs. A row holds
 * its own start and one start per document that begins inside it, and a document begins once
 * in the stream: a batch of distinct rows has at most batch + n_doc starts and at most batch *
 * L, so max_seqs = min(batch * L, batch + n_doc) cannot overflow (with repeated rows,
 * min(batch * L, batch * (1 + n_doc))). One workgroup, one launch.
 *
 * All three fail with -1 before anything is launched on seq_len outside [1, 2^20], a negative
 * size, and a NULL array of non-zero size; the plan and the rows on a rate outside [0, 65536];
 * the rows on a negative eos_id and on fim_q > 0 with any of the three sentinel ids negative;
 * lddl_stream_cu_seqlens on max_seqs < 1 and batch * seq_len > 2^31 - 1. batch = 0 writes no
 * row.
 * ------------------------------------------------------------------------------------------- */
#define LDDL_STREAM_TILE 1024
#define LDDL_STREAM_LDS_DOCS 256
int lddl_stream_plan(void* stream, const int32_t* d_sent_len, int64_t n_sent,
                     const int64_t* d_doc_sent_off, int64_t n_doc, const int64_t* d_doc_order,
                     int32_t seq_len, int32_t fim_q, int32_t spm_q, uint64_t seed,
                     uint64_t counter, int64_t* d_sent_tok_off, int64_t* d_doc_off,
                     int64_t* d_n_rows);
int lddl_stream_release(void);
int lddl_stream_rows(void* stream, const int32_t* d_ids, const int64_t* d_sent_off,
                     int64_t n_sent, const int64_t* d_doc_sent_off, int64_t n_doc,
                     const int64_t* d_doc_order, const int64_t* d_sent_tok_off,
                     const int64_t* d_doc_off, const int64_t* d_rows, int32_t batch,
                     int32_t seq_len, int32_t fim_q, int32_t spm_q, uint64_t seed,
                     uint64_t counter, int64_t eos_id, int64_t fim_prefix_id,
                     int64_t fim_middle_id, int64_t fim_suffix_id, int32_t eod_mask_loss,
                     int32_t reset_position_ids, int64_t ignore_index, int64_t* d_input_ids,
                     int64_t* d_labels, int64_t* d_position_ids, int64_t* d_sequence_ids);
int lddl_stream_cu_seqlens(void* stream, const int64_t* d_doc_off, int64_t n_doc,
                           const int64_t* d_rows, int32_t batch, int32_t seq_len,
                           int32_t max_seqs, int32_t* d_cu_seqlens, int32_t* d_n_seqs);

#ifdef __cplusplus
}
#endif

#endif /* LDDL_AMD_H_ */
