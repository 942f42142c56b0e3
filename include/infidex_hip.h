/*
 * infidex_hip.h — C ABI of libinfidex_hip.so: the MI355X (gfx950) drop-in for the query-time scoring hot path
 * of lofcz/Infidex (SearchEngine.Search -> SearchPipeline.Execute).
 *
 * The reference has no FFI seam today; the two INTERNAL calls this library replaces are
 *   S1  Bm25Scorer.Search(TermScoreInfo[] termInfos, int topK, int totalDocs, float[] docLengths, float avgdl, ...)
 *         -> TopKHeap                       src/Infidex/Indexing/Bm25Scorer.cs:56-67  (caller VectorModel.cs:567-569)
 *   S2  CoverageEngine.CalculateFeatures(ctx, docText, lcsSum, buffer, docId) + FusionScorer.Calculate(...)
 *         -> (float score, byte tiebreaker) src/Infidex/Coverage/CoverageEngine.cs:174, Scoring/FusionScorer.cs:19-25
 *                                           (caller SearchPipeline.ProcessCandidate, Scoring/SearchPipeline.cs:449-522)
 * A C# host binds these entry points with [DllImport("infidex_hip")] (stub in INTEGRATION.md).
 *
 * Conventions: every function returns an int32 status (0 = INFX_OK); no exceptions cross the ABI; the caller owns
 * all buffers; uploads are copied to HBM and host pointers are never retained; handles are opaque and freed only by
 * infx_destroy. infx_stage*_batch are re-entrant on an uploaded (immutable) index when each caller uses its own
 * infx_stream; infx_upload_* / infx_destroy are exclusive (the reference holds its write lock there,
 * SearchEngine.cs:96-104). Thread-local error text: infx_last_error().
 */
#ifndef INFIDEX_HIP_H
#define INFIDEX_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INFX_OK            0
#define INFX_EINVAL        1   /* bad argument / unsupported size */
#define INFX_ENOMEM        2   /* hipMalloc failed */
#define INFX_EHIP          3   /* HIP runtime error (incl. "no GPU") */
#define INFX_ECAPACITY     4   /* a per-batch workspace bound would be exceeded; split the batch */
#define INFX_EUNSUPPORTED  5   /* input outside the supported envelope (e.g. > INFX_MAX_DOC_TOKENS tokens) */
#define INFX_ENCCL         6   /* RCCL error (or librccl could not be loaded) */

#define INFX_MAX_QUERY_TERMS   128  /* VectorModel.cs:381 rents 128 raw tokens */
#define INFX_MAX_QUERY_TOKENS  32   /* Stage-2 query words after dedupe: the fast envelope (infx_cov_query) */
#define INFX_MAX_QUERY_CHARS   512
#define INFX_LONGQ_TOKENS      128  /* the long envelope (infx_cov_query_long): queries beyond the fast one take k_stage2's long-query launches — slower, same results */
#define INFX_LONGQ_CHARS       2048
#define INFX_MAX_DOC_TOKENS    192  /* Stage-2 words per document text handled in registers / scratch; longer texts (the reference allows 65 535 characters,
                                       Api/DocumentFields.cs:140) take k_stage2's global-workspace pass: slower, same results */
#define INFX_NFEAT             32   /* ints per infx_cov_out.feat */

typedef struct infx_index infx_index;     /* device-resident immutable index (one shard) */
typedef struct infx_stream infx_stream;   /* per-caller HIP stream + workspace */

/* Replaces the constants of Bm25Scorer.cs:21-23 / ConfigurationParameters.cs:101-104. */
typedef struct infx_config {
    int32_t device;          /* HIP device ordinal */
    int32_t range_docs;      /* documents per LDS range block (power of two, 512..16384); 0 = chosen from the shard size at
                                infx_upload_docs: 1024 below 256k documents ... 8192 from 4M documents */
    int32_t max_depth;       /* largest Query.CoverageDepth that will be used (default 500) */
    int32_t flags;           /* INFX_CFG_* */
} infx_config;
/* Queries whose Stage-1 top-`depth` cut is ambiguous (rows within a few ulp of each other around the cut, exact ties included) are
 * replayed with the reference's sequential semantics — chunked Vector256 / scalar-tail BM25 rounding (Bm25Scorer.cs:395-444) and the
 * BCL PriorityQueue eviction order (Bm25Scorer.cs:654-670) — by k_exact1, so the Stage-1 set and scores are the reference's bit for
 * bit.  This flag turns the replay off (the cut is then taken by (score, doc id)).  Document shards replay through infx_shard_replay_* (below). */
#define INFX_CFG_NO_EXACT_REPLAY 1

int32_t infx_create(const infx_config* cfg, infx_index** out);
void    infx_destroy(infx_index* idx);
const char* infx_last_error(void);

/* Postings: Term.docIds/weights (Core/Term.cs:21-22) flattened to CSR. df[t] < 0 marks a stop term (Term.cs:134-146);
 * its slice must be empty. doc ids are shard-local internal ids in ascending order. */
int32_t infx_upload_postings(infx_index* idx, uint32_t num_terms, const uint64_t* offs /* T+1 */,
                             const int32_t* doc_ids, const uint8_t* tf, const int32_t* df);

/* Documents: VectorModel._docLengths/_avgDocLength (VectorModel.cs:25-26, global avgdl!), DocumentKey, and the
 * Stage-2 text = ToLowerInvariant(TextNormalizer.Normalize(doc.IndexedText)) as UTF-16 (SegmentProcessor.cs:42-75;
 * every Stage-2 comparison in the reference is OrdinalIgnoreCase, so folding once at upload is equivalent). */
int32_t infx_upload_docs(infx_index* idx, uint32_t num_docs, const float* doc_len, float avgdl,
                         const int64_t* doc_key, const uint8_t* deleted /* N flags (Document.Deleted) or NULL; unsharded indexes only */,
                         const uint64_t* text_offs /* N+1 */, const uint16_t* text_utf16);

/* Document.Deleted (Core/Document.cs) after the upload: `deleted` holds one flag per GLOBAL internal id (`total_docs` of them — the same array on
 * every shard; NULL clears all flags).  Nothing else changes, exactly as in the reference between a deletion and the next re-index: postings, df,
 * doc lengths and avgdl keep the deleted documents.  The query path then skips them where the reference does — a deleted document is scored with
 * its chunk but never offered to the top-K heap (Bm25Scorer.cs:322-323, 455-459, 622-624), is not scored by Stage 2 (SearchPipeline.cs:463-465), and
 * a deleted WordMatcher id gets no docIndex (SearchPipeline.cs:532-537) while still counting against the WordMatcher-only limit (:387-397).
 * Call it while no search is in flight on this index (the reference mutates documents under its write lock). */
int32_t infx_set_deleted(infx_index* idx, uint32_t total_docs, const uint8_t* deleted);

/* Prefix DocSets (PrefixPostingList.DocSet, Indexing/ShortQuery/PrefixPosting.cs:64,109-137) that prefix precedence
 * can accept (population <= 20*max_depth), CSR over sets; referenced by set index from infx_query.prefix_set. */
int32_t infx_upload_prefix_docsets(infx_index* idx, uint32_t num_sets, const uint64_t* offs, const int32_t* doc_ids);

/* Document-sharded operation: this index holds internal ids [doc_base, doc_base+num_docs) of a corpus
 * of total_docs; corpus statistics passed in queries are global. */
int32_t infx_set_shard(infx_index* idx, int32_t rank, int32_t nranks, int32_t doc_base, int32_t total_docs);

/* RCCL inside the boundary (infx_set_shard(..., ncclUniqueId)).  Rank 0 creates the 128-byte ncclUniqueId and ships it to every rank
 * (any transport); every rank then joins the communicator of its index (ncclCommInitRank(nranks, id, rank) on the index's device, after infx_set_shard).
 * The collectives below are enqueued on the stream's HIP stream over DEVICE buffers — stream-ordered behind the kernels that produced the data and in
 * front of the ones that consume it, no host synchronisation: count all-reduce (Exchange 1 / 1b), all-gather of the per-shard top-k (Exchange 2).
 * librccl is loaded with dlopen at the first call: an unsharded deployment does not need it. */
#define INFX_RCCL_ID_BYTES 128
int32_t infx_rccl_unique_id(void* id128);
int32_t infx_set_shard_comm(infx_index* idx, const void* id128);
/* a communicator of its own for one stream (another ncclUniqueId; same call order on every rank): batches in flight on different streams then exchange
 * without serialising on one communicator.  A stream without one uses the index's. */
int32_t infx_stream_comm(infx_stream* s, const void* id128);
int32_t infx_comm_allreduce_sum_u32(infx_stream* s, void* buf /* device, in place */, uint64_t count);
int32_t infx_comm_allgather(infx_stream* s, const void* send /* device */, void* recv /* device: nranks x bytes_per_rank */, uint64_t bytes_per_rank);
/* Plumbing for a native host driver of the sharded phases (infidex_engine.h: infx_session_sharded_finish): per-stream device scratch buffers (slot < 16,
 * grown on demand, valid until the next call with the same slot), copies between host and device memory of either kind, stream synchronisation. */
int32_t infx_stream_scratch(infx_stream* s, int32_t slot, uint64_t bytes, void** out);
int32_t infx_stream_copy(infx_stream* s, void* dst, const void* src, uint64_t bytes);      /* stream-ordered; host pointers are staged; call infx_stream_wait before reading a host destination */
int32_t infx_stream_fill0(infx_stream* s, void* dev, uint64_t bytes);
/* After an all-gather of ONE packed block per rank (parts of part_bytes[p] bytes back to back, blocks `stride` bytes apart): dsts[p] receives the nranks
 * pieces of part p consecutively (rank-major), as separate all-gathers of the parts would have left them.  Device memory: a stream-ordered kernel; host: memcpy. */
int32_t infx_stream_unpack(infx_stream* s, const void* src, uint64_t stride, int32_t nranks, int32_t nparts /* <= 4 */, const uint64_t* part_bytes, void* const* dsts);
int32_t infx_stream_wait(infx_stream* s);
int32_t infx_stream_native(infx_stream* s, void** hip_stream);      /* the hipStream_t the stream's kernels, copies and collectives are ordered on */
/* The HIP streams this stream object launches on, by priority.  The runtime serves streams from a small pool of hardware queues and streams beyond the pool
 * share one: normal = 1 (the hot path, one of the index's INFX_MAIN_STREAMS main streams), 2 with INFX_REPLAY_AUX=1 (the replay's k_ex_chunk launches side by
 * side, on a stream of its own); high = 1 (planning) where the device offers stream priorities and INFX_PLAN_PRIORITY is not 0.  The main stream is shared with other
 * infx_streams once more of them exist on the device than the pool has streams (infx_stream_native tells which): they run in order on it, and event timings on it span
 * each other's kernels. */
int32_t infx_stream_budget(infx_stream* s, int32_t* normal, int32_t* high);

int32_t infx_stream_create(infx_index* idx, infx_stream** out);
void    infx_stream_destroy(infx_stream* s);

/* ---- Stage 1 ------------------------------------------------------------------------------------------------- */
/* One term of a query, in Bm25Scorer order (ascending termId; fuzzy virtual terms first — VectorModel.cs:442). */
typedef struct infx_term {
    int32_t  term_id;      /* >= 0: index term; -1: virtual (fuzzy-union) term, postings in the batch's extra arrays */
    uint32_t extra_off;    /* virtual term: offset into infx_stage1_batch.extra_docs; its tf == 1 (RoaringPostingsEnum.cs:21) */
    uint32_t extra_len;
    float    idf;          /* Bm25Scorer.ComputeIdf on the host (MathF.Log), Bm25Scorer.cs:686-695 */
    float    max_score;    /* VectorModel.cs:525-531 */
    uint8_t  role;         /* INFX_ROLE_* bits: membership in the candidate tiers */
    uint8_t  rank;         /* disjunctive: position in the IDF-descending order among eligible terms (TieredCandidateSelector.cs:253) */
    uint16_t reserved;     /* virtual term only: 0 = extra_docs[extra_off..+len) are the union's doc ids (shard-local, ascending);
                              1 = they are the MEMBER TERM IDS (<= LD1 matches, VectorModel.cs:660-683): the union is formed on the
                              device inside the accumulate launch (one posting stream per member, each document counted once);
                              2 = extra_off is the index of a union materialised on the device by the last infx_union_build */
} infx_term;

#define INFX_ROLE_AND      1   /* AND mode: member of terms[0..n-2] (everything but the lowest-IDF term) */
#define INFX_ROLE_LOWEST   2   /* AND mode: the lowest-IDF term (dropped by Tier 1)                      */
#define INFX_ROLE_S1       4   /* AND mode: first selective term of Tier 2                               */
#define INFX_ROLE_S2       8   /* AND mode: second selective term of Tier 2                              */
#define INFX_ROLE_ELIGIBLE 16  /* disjunctive: not low-quality (idf >= 0.2*maxIdf)                       */
#define INFX_ROLE_LOWQ     32  /* disjunctive: low-quality term (only used when nothing selective hit)   */

#define INFX_MODE_PREFIX   1   /* candidates = accepted prefix DocSet alone (TieredCandidateSelector.cs:66-82)   */
#define INFX_MODE_DISJ     2   /* SelectCandidatesDisjunctive (:108-125, :243-322)                               */
#define INFX_MODE_AND      3   /* Tier 0/1/2 (:128-234)                                                          */

typedef struct infx_query {
    uint32_t term_off;     /* into the batch's terms[] */
    uint32_t num_terms;
    int32_t  mode;         /* INFX_MODE_* (decided on the host from global df / DocSet populations) */
    int32_t  prefix_set;   /* MODE_PREFIX: the candidate set; other modes: set of pre-"seen" docs (< min(2k,100) docs) or -1 */
    int32_t  depth;        /* topK handed to Bm25Scorer.Search == Query.CoverageDepth (SearchPipeline.cs:282) */
    int32_t  n_and;        /* AND mode: number of terms (n); needed for the Tier-0 / Tier-1 membership tests */
    int32_t  df_s1;        /* AND mode: global df of S1 / S2 (Tier-2 cardinality tests, :221) */
    int32_t  df_s2;
} infx_query;

typedef struct infx_hit { int32_t doc; float score; } infx_hit;   /* doc = global internal id; key via infx_upload_docs */

/* Per-query class counts of the candidate tiers on THIS shard (sum over shards before infx_stage1_select when sharded).
 * A document is counted when a candidate-generating list of the query holds it and its accumulated score is > 0 (a term with idf <= 0 adds nothing; a
 * document hit by such terms alone is no row and is not counted).  Deleted documents ARE counted: the reference's tiers see them.  c[] by infx_query.mode:
 *   INFX_MODE_AND     c[0..15], index = bit 0: the document holds every INFX_ROLE_AND term and the INFX_ROLE_LOWEST one (Tier 0)
 *                                     | bit 1: it holds every INFX_ROLE_AND term and n_and >= 3 (Tier 1; contains Tier 0)
 *                                     | bit 2: it is in the list of INFX_ROLE_S1 | bit 3: ... of INFX_ROLE_S2.
 *                     Only documents of S1 u S2 are counted (index >= 4): Tier 0 and Tier 1 lie inside S1, the term of the highest idf.
 *   INFX_MODE_DISJ    c[r], r < 128: documents whose smallest infx_term.rank among the INFX_ROLE_ELIGIBLE / INFX_ROLE_LOWQ terms that hold them is r
 *                     (localCount of SelectCandidatesDisjunctive per term).  Documents of the query's pre-"seen" set (prefix_set) are not counted.
 *   INFX_MODE_PREFIX  c[1]: documents of the prefix DocSet with a score > 0.
 * Every other entry is 0 (c[128..135] are reserved).  infx_stage1_select reads the tier rules off these counts: which tiers the reference would have
 * unioned (AND), up to which rank its walk would have gone (DISJ). */
#define INFX_NCLASS 136
typedef struct infx_counts { uint32_t c[INFX_NCLASS]; } infx_counts;

/* Stage 1a: stream postings, accumulate BM25+ in LDS, emit candidate supersets + class counts (device resident). */
int32_t infx_stage1_accumulate(infx_stream* s, uint32_t nq, const infx_query* q, uint32_t nterms, const infx_term* terms,
                               uint32_t extra_n, const int32_t* extra_docs, infx_counts* counts_out /* nq; host memory or a device buffer */);
/* Stage 1b: apply the tier rules with (global) counts, select the top-`depth` per query ordered by
 * (score desc, DocumentKey asc). out: nq*depth hits; out_count: nq. Replaces UpdateTopK/PriorityQueue (Bm25Scorer.cs:654-670). */
int32_t infx_stage1_select(infx_stream* s, uint32_t nq, const infx_counts* counts /* nq, host, global */,
                           infx_hit* out, uint32_t* out_count);
/* Convenience for the unsharded case: accumulate + select. == Bm25Scorer.Search for a batch of queries. */
int32_t infx_stage1_batch(infx_stream* s, uint32_t nq, const infx_query* q, uint32_t nterms, const infx_term* terms,
                          uint32_t extra_n, const int32_t* extra_docs, infx_hit* out, uint32_t* out_count);

/* Fuzzy virtual terms on the device (ExpandMissingTerm, VectorModel.cs:643-743): for v in [0, nv) the union of the doc sets of
 * members[member_offs[v] .. member_offs[v+1]) is materialised in HBM (ascending, shard-local ids) and counts_out[v] = its
 * cardinality on this shard (RoaringBitmap.Cardinality, :722-729; sum over shards for the global df — Exchange 1b). The unions stay
 * valid on this stream until the next infx_union_build and are referenced by infx_term {term_id -1, reserved 2, extra_off v}. */
int32_t infx_union_build(infx_stream* s, uint32_t nv, const uint32_t* member_offs, const int32_t* members, uint32_t* counts_out);

/* ---- Stage 2 ------------------------------------------------------------------------------------------------- */
/* CoverageQueryContext (Coverage/CoverageEngine.cs:9-43) of one query, prepared on the host (PrepareQuery :61-126). */
typedef struct infx_cov_query {
    uint16_t text[INFX_MAX_QUERY_CHARS];          /* normalised, lower-cased query */
    int32_t  text_len;
    int32_t  num_tokens;                          /* deduplicated, MinWordSize-filtered */
    uint16_t tok_off[INFX_MAX_QUERY_TOKENS];
    uint16_t tok_len[INFX_MAX_QUERY_TOKENS];
    float    term_idf[INFX_MAX_QUERY_TOKENS];     /* n-gram averaged (ComputeTermIdf :388-427) */
    float    word_idf[INFX_MAX_QUERY_TOKENS];     /* WordIdfCache (VectorModel.cs:864-908), 0 when absent */
    int32_t  has_word_idf;
    int32_t  num_fusion_tokens;                   /* unfiltered tokens (minWordSize 0), CoverageEngine.cs:348-352 */
    uint16_t ftok_off[INFX_MAX_QUERY_TOKENS * 2];
    uint16_t ftok_len[INFX_MAX_QUERY_TOKENS * 2];
    int32_t  lcs_tolerance;                       /* SearchPipeline.cs:498-500 */
    int32_t  reserved;                            /* 0, or 1 + the index of this query's record in the stream's long-query table (infx_stage2_long_queries): the
                                                     query is beyond the fast envelope, lives there, and the other members of this struct are ignored */
} infx_cov_query;
/* The same context for a query beyond INFX_MAX_QUERY_TOKENS distinct words / INFX_MAX_QUERY_CHARS characters (the reference has no limit: PrepareQuery rents
 * query.Length / 2 + 1 token slots, CoverageEngine.cs:68): up to INFX_LONGQ_TOKENS / INFX_LONGQ_CHARS.  Same members, larger tables. */
typedef struct infx_cov_query_long {
    uint16_t text[INFX_LONGQ_CHARS];
    int32_t  text_len;
    int32_t  num_tokens;
    uint16_t tok_off[INFX_LONGQ_TOKENS];
    uint16_t tok_len[INFX_LONGQ_TOKENS];
    float    term_idf[INFX_LONGQ_TOKENS];
    float    word_idf[INFX_LONGQ_TOKENS];
    int32_t  has_word_idf;
    int32_t  num_fusion_tokens;
    uint16_t ftok_off[INFX_LONGQ_TOKENS * 2];
    uint16_t ftok_len[INFX_LONGQ_TOKENS * 2];
    int32_t  lcs_tolerance;
    int32_t  reserved;
} infx_cov_query_long;

typedef struct infx_cov_cand {
    uint32_t query;        /* index into the batch's infx_cov_query[] */
    int32_t  doc;          /* shard-local internal id */
    float    base_score;   /* normBm25 = s / s_top1, or 0 for WordMatcher candidates (SearchPipeline.cs:380-414) */
    int32_t  want_lcs;     /* 1 for docIndex < 2 (quirk Q7, SearchPipeline.cs:492-503); 2: the same document's SECOND evaluation (its Stage-1 row after its WordMatcher
                              overlap row): the reference reads the LCS back from a byte span there, so a value above 255 comes back as 255 (quirk Q18, :494-503) */
} infx_cov_cand;

typedef struct infx_cov_out {
    float   score;         /* FusionScorer.Calculate: (float)precedence + semantic */
    uint8_t tiebreaker;
    uint8_t word_hits;     /* min(WordHits,255) */
    uint8_t lcs;           /* min(lcs,255) when want_lcs */
    uint8_t status;        /* 0 ok; INFX_EUNSUPPORTED: the over-long documents (> INFX_MAX_DOC_TOKENS words) of one launch exceeded the 64 MB token-table pool */
    int32_t word_hits_full;
} infx_cov_out;

/* feat_out (may be NULL): ncand x INFX_NFEAT ints — CoverageFeatures / FusionSignals (the bit-exact parity target; the
 * reference keeps them internal, Coverage/CoverageFeatures.cs:3-88), layout in DESIGN.md. */
/* Long queries of the NEXT Stage-2 call on this stream (infx_stage2_batch, infx_search_fused, infx_shard_stage2): n records, referred to by
 * infx_cov_query.reserved = 1 + index.  The table is consumed by that call; n = 0 clears it. */
int32_t infx_stage2_long_queries(infx_stream* s, uint32_t n, const infx_cov_query_long* q);
/* CoverageSetup (Coverage/CoverageSetup.cs) on the device.  infx_stage2_setup: the ENGINE-WIDE matcher settings — CoverageEngine._setup, CoverageEngine.cs:71,269,
 * 323-341,378 and FuzzyWordMatcher.cs:14-144; min_word_size is also minStemLength of the fusion signals; cover_prefix_suffix off also means that k_wm looks up
 * no affix matches (WordMatcherLookup.cs:51).  Values in [0, 65535]; num_typos above 2 behaves as 2 (the reference's formula never asks for more).
 * infx_finalize_setup: what ResultProcessor.CalculateTruncationIndex (ResultProcessor.cs:151-171) and SearchPipeline.cs:425,433 read, one record PER QUERY.
 * infx_stream_set_coverage hands both to the stream: `matchers` (NULL = CoverageSetup's defaults) to the NEXT Stage-2 call (infx_stage2_batch, infx_search_fused,
 * infx_shard_stage2, infx_wm_lookup_debug), `per_query` (nq records, NULL = the defaults for every query) to the NEXT finalize (infx_search_fused,
 * infx_shard_finalize); each consumes its part, and a call replaces whatever an earlier one left.  Matcher settings that differ from the defaults run the
 * "custom setup" instantiations of k_stage2 (the settings as kernel arguments; six more kernels); the defaults keep the instantiations in which they are compile-time constants. */
typedef struct infx_stage2_setup {
    int32_t min_word_size, lev_max_word_size, num_typos, min_len_one_typo, min_len_two_typos;                       /* 2, 20, 2, 3, 7 */
    int32_t cover_whole_query, cover_whole_words, cover_fuzzy_words, cover_joined_words, cover_prefix_suffix;        /* 1 each */
} infx_stage2_setup;
typedef struct infx_finalize_setup {
    int32_t truncate;                                 /* Truncate: 1 */
    int32_t min_hits_abs, min_hits_relative;          /* CoverageMinWordHitsAbs 1, CoverageMinWordHitsRelative 0 */
    int32_t truncation_score;                         /* TruncationScore 254, in [0, 255] */
} infx_finalize_setup;
int32_t infx_stream_set_coverage(infx_stream* s, const infx_stage2_setup* matchers, uint32_t nq, const infx_finalize_setup* per_query);
int32_t infx_stage2_batch(infx_stream* s, uint32_t nq, const infx_cov_query* q, uint32_t ncand,
                          const infx_cov_cand* cand, infx_cov_out* out, int32_t* feat_out);

/* ---- Infiscript post-filter + facet aggregation on device-resident columns (BASELINE config 5) ---------------------------------------
 * Replaces ResultProcessor.ApplyFilter (Scoring/ResultProcessor.cs:35-70: FilterVM.Execute per returned row, and over ALL documents for
 * Filter.NumberOfDocumentsInFilter on first use) and FacetBuilder.BuildFacets (Core/FacetBuilder.cs:19-105) for the rows a search returns.
 * A column = one non-indexed document field, dictionary-encoded by the host: codes[d] = index of document d's value among the field's
 * distinct values (GLOBAL internal ids: every shard holds the whole column, 4 B per document).
 * A filter = a postfix program over LEAVES; leaf l is a bitmap over the codes of column leaf.col (bit v = "the leaf's predicate holds for
 * distinct value v", evaluated by the host with FilterVM's coercion rules); three-valued evaluation F / T / N as in the reference's
 * untyped VM: AND(l,r) = l==F ? F : r, OR(l,r) = l==T ? T : r, NOT(x) = x==T ? F : T, TERN(c,a,b) = c==F ? b : a, LIT = N; match iff T. */
typedef struct infx_filter infx_filter;
#define INFX_FOP_LEAF 0
#define INFX_FOP_AND  1
#define INFX_FOP_OR   2
#define INFX_FOP_NOT  3
#define INFX_FOP_TERN 4
#define INFX_FOP_LIT  5
#define INFX_FILTER_MAX_OPS 256
#define INFX_FILTER_MAX_ROWS 64         /* post-filter / facets run on <= 64 returned rows per query (Query.MaxNumberOfRecordsToReturn) unless the index is configured for more */
#define INFX_POST_MAX_ROWS 1024         /* the most rows per query an index can be configured to post-process (infx_set_post_rows): SEL_CAP / 2, the largest max_depth */
#define INFX_MAX_FACET_COLS 8
typedef struct infx_filter_op { uint32_t op; uint32_t arg; } infx_filter_op;                 /* arg: leaf index for INFX_FOP_LEAF */
typedef struct infx_filter_leaf { uint32_t col; uint32_t table_off; uint32_t num_values; uint32_t reserved; } infx_filter_leaf;   /* col 0xFFFFFFFF: no such field (null) */
/* Post rows of the index: how many returned rows per query the post-filter, facets, boosts, sort-by and browse rows accept, INFX_FILTER_MAX_ROWS (the
 * default) .. INFX_POST_MAX_ROWS.  A query with post-processing that asks for at most INFX_FILTER_MAX_ROWS rows runs on the one-wave kernels whatever the
 * setting; one that asks for more, up to the post rows, runs on workgroup-per-query kernels (k_postfilter_wide, k_postproc_wide, k_browse_rows_wide) that
 * are launched only for a batch that has such a query.  The post rows are also the stride of the facet pairs of infx_last_facets.  Exclusive call, between
 * searches (as infx_upload_column). */
int32_t infx_set_post_rows(infx_index* idx, int32_t rows);
int32_t infx_get_post_rows(infx_index* idx, int32_t* rows);
int32_t infx_upload_column(infx_index* idx, uint32_t col, uint32_t total_docs, const uint32_t* codes, uint32_t num_values);
int32_t infx_filter_create(infx_index* idx, uint32_t nops, const infx_filter_op* ops, uint32_t nleaves, const infx_filter_leaf* leaves,
                           uint32_t ntable_words, const uint32_t* tables, infx_filter** out);
void    infx_filter_destroy(infx_filter* f);
/* The validation infx_filter_create and the per-query program tables apply, on its own: INFX_OK, or the status and message they would refuse the program with
 * (more than INFX_FILTER_MAX_OPS ops, a stack deeper than the kernels' 32 slots, a malformed program, a column that was not uploaded).  Touches no device. */
int32_t infx_filter_check(infx_index* idx, uint32_t nops, const infx_filter_op* ops, uint32_t nleaves, const infx_filter_leaf* leaves, uint32_t ntable_words);
/* Documents of THIS shard the filter accepts (sum over shards = Filter.NumberOfDocumentsInFilter): k_filter_count_multi with K = 1. */
int32_t infx_filter_count(infx_stream* s, infx_filter* f, uint32_t* count);
/* Installs (f != NULL) or clears the post-filter and the facet columns of this stream: every following infx_search_fused /
 * infx_shard_finalize filters its result rows on the device before they are returned and counts the facet values of the kept rows. */
int32_t infx_stream_set_postfilter(infx_stream* s, infx_filter* f, uint32_t nfacet, const uint32_t* facet_cols);
/* Facets of the last search on this stream: for query q and facet column k, n_out[q*nfacet+k] pairs at codes_out / counts_out
 * [(q*nfacet+k)*R ..], R = the index's post rows (infx_get_post_rows; INFX_FILTER_MAX_ROWS unless set), in row order of first occurrence (the host orders them: count desc, value asc). */
int32_t infx_last_facets(infx_stream* s, uint32_t nq, uint32_t* codes_out, uint32_t* counts_out, uint32_t* n_out);
/* ... of query q and facet column k alone: *n_out pairs (at most the index's post rows) at codes_out / counts_out */
int32_t infx_last_facets_of(infx_stream* s, uint32_t nq, uint32_t q, uint32_t k, uint32_t* codes_out, uint32_t* counts_out, uint32_t* n_out);

/* ---- Query.Boosts + Query.SortBy on the returned rows (k_postproc) ----------------------------------------------------------------------
 * Replaces ResultProcessor.ApplyBoosts / ApplySort (Scoring/ResultProcessor.cs:75-141, 180-201) as SearchEngine.ApplyPostProcessing calls them
 * after ApplyFilter (SearchEngine.cs:348-361).  Installed on a stream, they apply to every following infx_search_fused / infx_shard_finalize,
 * after the post-filter, on at most the index's post rows per query (INFX_FILTER_MAX_ROWS unless infx_set_post_rows raised them; more: INFX_EUNSUPPORTED).  Both steps end in the BCL's unstable
 * introsort (Array.Sort with a Comparison), replayed on the device, so rows that compare equal come back in the reference's order. */
#define INFX_MAX_BOOSTS 8
/* Sort rank of column col: rank[v] for each of its num_values distinct values (codes), dense — equal values share a rank — in the order of
 * CompareValues (the host encodes the value semantics: numbers, NaN lowest, -0 == +0, strings).  num_values must be the column's. */
int32_t infx_upload_sort_rank(infx_index* idx, uint32_t col, uint32_t num_values, const uint32_t* rank);
/* Query.Boosts with Query.EnableBoost: n boosts, f[i] its filter (NULL: a Boost whose Filter is null, dropped), strengths[i] = (int)BoostStrength.
 * At most INFX_MAX_BOOSTS with a filter (INFX_ECAPACITY).  Once one with a filter is installed, the rows are re-sorted by score descending even
 * when no row was boosted.  n = 0 clears. */
int32_t infx_stream_set_boosts(infx_stream* s, uint32_t n, infx_filter* const* f, const int32_t* strengths);
/* Query.SortBy / Query.SortAscending: sort the rows by column col (0xFFFFFFFF: no such field — every row null, the sort still permutes rows);
 * enabled = 0 clears.  The column's sort rank must have been uploaded. */
int32_t infx_stream_set_sort(infx_stream* s, uint32_t col, int32_t ascending, int32_t enabled);

/* ---- per-query post-processing: a batch of Query objects, each with its own Filter / EnableFacets / Boosts / SortBy ----------------------------
 * infx_stream_set_query_post installs the options of the NEXT batch on the stream (one infx_search_fused, or the infx_shard_finalize of the next
 * sharded batch); that batch consumes them.  progs: the batch's distinct filter programs (host memory, copied: packed into one blob that is staged
 * with the batch, nothing is allocated per program); boosts: the batch's boost list, each entry a program index + (int)BoostStrength; post[q]: query
 * q's descriptor — filter = program index or -1, flags INFX_QP_*, sort_col = column (0xFFFFFFFF: no such field, every row null), boosts
 * [boost_off, + nboost) with nboost <= INFX_MAX_BOOSTS.  nfacet / facet_cols: the columns a query with INFX_QP_FACETS counts (infx_last_facets;
 * 0 pairs for the queries without).  A query without filter, facets, boosts or sort passes through unchanged, whatever its number of rows; a query
 * with post-processing whose rows exceed the index's post rows (INFX_FILTER_MAX_ROWS by default) comes back empty with result flag INFX_RESULT_REJECTED (the others of the batch are
 * unaffected).  ncount: programs [0, ncount) are counted over every document of the corpus that is not Deleted (Filter.NumberOfDocumentsInFilter,
 * whole corpus on every shard: each holds the whole columns and the global Deleted flags) by k_filter_count_multi, enqueued with the batch: the
 * counts land in counts_out when the batch's results do.  Exclusive with infx_stream_set_postfilter / _set_boosts / _set_sort (INFX_EINVAL); the
 * session-wide setters are the case of one descriptor every query shares, on the same kernels.  nq = 0 clears; a batch of another size fails. */
#define INFX_QP_FACETS 1u
#define INFX_QP_SORT   2u
#define INFX_QP_ASC    4u
#define INFX_RESULT_REJECTED 16u        /* result flag bit 4: the query's post-processing was refused (see above / infx_engine_set_query_options) */
typedef struct infx_filter_prog { const infx_filter_op* ops; const infx_filter_leaf* leaves; const uint32_t* tables; uint32_t nops, nleaves, ntable_words, reserved; } infx_filter_prog;
typedef struct infx_query_boost { int32_t prog; int32_t strength; } infx_query_boost;
typedef struct infx_query_post { int32_t filter; uint32_t flags; uint32_t sort_col; uint32_t boost_off; uint32_t nboost; uint32_t reserved[3]; } infx_query_post;
int32_t infx_stream_set_query_post(infx_stream* s, uint32_t nq, uint32_t nprog, const infx_filter_prog* progs, uint32_t nboost, const infx_query_boost* boosts,
                                   const infx_query_post* post, uint32_t nfacet, const uint32_t* facet_cols, uint32_t ncount, uint32_t* counts_out);
/* k programs counted in one k_filter_count_multi launch (several past 4096 programs), synchronously: counts[i] = documents not Deleted that progs[i]
 * accepts — this shard's documents (whole_corpus = 0, as infx_filter_count) or every document of the corpus (1). */
int32_t infx_filter_count_progs(infx_stream* s, uint32_t k, const infx_filter_prog* progs, int32_t whole_corpus, uint32_t* counts);
/* the programs the last finalize (or infx_filter_count_progs) on this stream counted, and in how many k_filter_count_multi launches (0 when a batch's
 * browse scan counted them, see below) */
int32_t infx_last_filter_count_stats(infx_stream* s, uint32_t* counted, uint32_t* launches);

/* ---- pre-filter masks: rank only the documents a filter accepts ---------------------------------------------------------------------------
 * A query with a pre-filter P returns what it would return on the same index if every document P does not accept carried Document.Deleted: the
 * query reads a MASK — one byte per GLOBAL internal id, mask[g] = Deleted(g) || !accept_P(g) — wherever it would read the index's Deleted flags
 * (Stage-1 emission, the exact replay, the WordMatcher-only candidates).  Index statistics are untouched, as with deletions; the count, browse and
 * whole-corpus facet kernels keep the real flags.  Queries read masks on unsharded indexes only (infx_search_fused); a sharded index may build them for
 * infx_list_ordered, which reads them by global id.
 *   infx_stream_mask_slot   the device buffer of mask slot `slot` (< INFX_MAX_PREFILTERS) of this stream: total_docs bytes padded to a multiple of four,
 *                           allocated on first use, owned by the stream.  What a slot holds is the caller's bookkeeping.
 *   infx_filter_masks       stages the build of k (<= INFX_MAX_PREFILTERS) masks: masks[i] (device, as from infx_stream_mask_slot) receives the mask of
 *                           progs[i], counts[i] (host) the number of live documents it accepts.  The build is ONE k_filter_mask_multi launch over the
 *                           whole corpus, enqueued on the stream in front of its next infx_search_fused — no host wait of its own: the counts land when
 *                           that batch's results do — or by infx_stream_wait, whichever comes first.  k = 0 drops a staged build.
 *   infx_stream_set_doc_masks  the flags of each query of the stream's NEXT infx_search_fused of nq queries: masks[i] (device), or NULL = the index's
 *                           Deleted flags.  Consumed by that batch, whatever its outcome; nq = 0 clears; a batch of another size fails.
 *   infx_last_filter_mask_stats  masks built and k_filter_mask_multi launches of the last build on this stream. */
#define INFX_MAX_PREFILTERS 16
int32_t infx_stream_mask_slot(infx_stream* s, uint32_t slot, uint8_t** out);
int32_t infx_filter_masks(infx_stream* s, uint32_t k, const infx_filter_prog* progs, uint8_t* const* masks, uint32_t* counts);
int32_t infx_stream_set_doc_masks(infx_stream* s, uint32_t nq, const uint8_t* const* masks);
int32_t infx_last_filter_mask_stats(infx_stream* s, uint32_t* built, uint32_t* launches);

/* ---- collapsing: at most `keep` ranked rows per group (not in the reference; DESIGN.md "collapse_by") ------------------------------------------------
 * infx_stream_set_query_collapse installs one request per query of the stream's NEXT finalize of nq queries (infx_search_fused): col < 0 = the query is not
 * collapsed, else the column whose dictionary code is a row's group (uploaded, covering the corpus) and keep in 1 .. INFX_COLLAPSE_MAX_KEEP.  Consumed by that
 * batch, whatever its outcome; nq = 0 clears; a batch of another size fails with INFX_EINVAL.  The depth of such a batch is at most 1024.
 * A collapsing query's ranked list L is what the same query returns with max_results = depth and nothing else installed (consolidated, cut at the truncation
 * index, the Stage-1 rows where coverage returned nothing).  A row of L is kept when fewer than `keep` earlier rows of L carry the code of its document; the
 * query returns the first max_results kept rows, in L's order, and the post-filter, facets, boosts and sort-by run on those.  k_finalize writes L into a window
 * of the stream's scratch, ONE k_collapse launch (a workgroup per collapsing query) writes the kept rows at the caller's stride: the caller's buffers do not
 * grow.  A batch without a request launches exactly what it launched before.  Positions and integer adds only: the same bytes from any stream and placement.
 *   infx_last_collapse        per query of the last batch (nq: its size) the distinct groups of L and the rows of L; 0 for a query that was not collapsed
 *   infx_collapse_rows        query qi's returned rows, as the post-processing left them: each row's group code and the size of its group in L; returns the
 *                             rows written (at most cap), -1 on error
 *   infx_last_collapse_stats  collapsing queries and k_collapse launches of the stream's last finalize
 *   infx_last_collapse_timings  ms2[0] k_finalize's and ms2[1] k_collapse's duration in that finalize (HIP events; zeros when nothing was collapsed) */
#define INFX_COLLAPSE_MAX_KEEP 16
typedef struct infx_collapse_req { int32_t col; int32_t keep; } infx_collapse_req;
int32_t infx_stream_set_query_collapse(infx_stream* s, uint32_t nq, const infx_collapse_req* reqs);
int32_t infx_last_collapse(infx_stream* s, uint32_t nq, uint32_t* total_groups, uint32_t* total_ranked);
int32_t infx_collapse_rows(infx_stream* s, uint32_t qi, uint32_t* codes, uint32_t* sizes, int32_t cap);
int32_t infx_last_collapse_stats(infx_stream* s, uint32_t* queries, uint32_t* launches);
int32_t infx_last_collapse_timings(infx_stream* s, float* ms2);

/* ---- highlighting: where each returned document matched, the spans to paint, a snippet (not in the reference; DESIGN.md "highlight") -----------------
 * infx_stream_set_query_highlight installs one width per query of the stream's NEXT finalize of nq queries (infx_search_fused): 0 = the query does not ask,
 * else its snippet width in UTF-16 units, INFX_HIGHLIGHT_MIN_CHARS .. INFX_HIGHLIGHT_MAX_CHARS.  Installed BEFORE the batch (its Stage-2 call notes the matcher
 * settings, the alias flag and the queries' word counts for it), consumed by the batch, whatever its outcome; nq = 0 clears; a batch of another size fails
 * with INFX_EINVAL.  After k_postproc, ONE k_highlight launch — a lane per (query, row) slot of the result table, idle where the row is past the query's count
 * or the query did not ask — re-runs Stage 2's four matchers over the stored text of each returned row's document with the batch's infx_cov_query table,
 * infx_stage2_setup and alias flag, and writes per row: its status (0 ok, 1 the document has more than INFX_MAX_DOC_TOKENS words, 2 the query is outside the
 * fast envelope), per query word what matched it, the spans, and the snippet (row layout, span walk and window rule: csrc/highlight.h).  The rows are strided by
 * what the batch asked — its largest word count, its largest width — and come back with the batch's outputs.  A batch without a request launches and downloads
 * exactly what it did before.
 *   infx_highlight_layout        rows of query qi, the batch's term stride and snippet stride
 *   infx_highlight_rows          query qi's rows as returned, hl_row_u16(term stride, snippet stride) uint16 each; returns the rows written, -1 on error
 *   infx_last_highlight_stats    asking queries and k_highlight launches of the stream's last finalize: (k, 1), or (0, 0)
 *   infx_last_highlight_timings  k_highlight's duration in that finalize (HIP events; 0 when nothing was highlighted) and the bytes of rows downloaded */
#define INFX_HIGHLIGHT_MIN_CHARS 16
#define INFX_HIGHLIGHT_MAX_CHARS 512
#define INFX_HIGHLIGHT_MAX_SPANS 64
int32_t infx_stream_set_query_highlight(infx_stream* s, uint32_t nq, const int32_t* chars);
int32_t infx_highlight_layout(infx_stream* s, uint32_t qi, int32_t* rows, int32_t* term_stride, int32_t* snippet_stride);
int32_t infx_highlight_rows(infx_stream* s, uint32_t qi, uint16_t* out, int64_t cap_u16);
int32_t infx_last_highlight_stats(infx_stream* s, uint32_t* queries, uint32_t* launches);
int32_t infx_last_highlight_timings(infx_stream* s, float* ms, uint64_t* bytes);

/* ---- browse rows: a query with no text and EnableFacets (SearchEngine.HandleEmptyQueryWithFacets, SearchEngine.cs:321-346) -------------------------
 * A fused query flagged INFX_FQ_SKIP | INFX_FQ_BROWSE returns the first max_results (<= the index's post rows, else INFX_EUNSUPPORTED) documents in
 * internal order that are not Deleted and that its filter accepts — the filter of its infx_query_post descriptor (which must carry INFX_QP_FACETS) or
 * the stream's post-filter (with facet columns installed) — each with score 65535 and tiebreaker 0; result flags 0.  The rows are written where a text
 * query's rows land before the post-filter, so the facets of infx_last_facets are those of the rows.  All browse queries of a batch are grouped by
 * program and answered by one ordered scan of the whole corpus (every shard holds the whole columns: each rank computes the same rows, no collective);
 * when the batch has one, that scan also produces the ncount counts of infx_stream_set_query_post and k_filter_count_multi is not launched.
 * The output order is the document order by construction (per-range counts, a prefix, ballot compaction): it does not vary from run to run.
 * infx_set_first_live: first[d] = first live document carrying document d's key, one entry per GLOBAL internal id; a browse row's filter and facets
 * look at that document (ResultProcessor.ApplyFilter / FacetBuilder look a row up by key), while the counts evaluate each document's own fields.
 * Needed only for a corpus with duplicate keys, to be refreshed when Deleted flags change; NULL clears; infx_upload_docs and a change of total_docs
 * (infx_set_shard) void it.  Exclusive call, as infx_set_deleted.
 * A group that only needs rows (count cached, or no filter) stops inside a range of the scan once the range holds enough matches; the environment
 * variable INFX_BROWSE_EARLY_STOP=0, read once per process, switches that off for measurements (tools/bench_browse.py) — the results do not change. */
int32_t infx_set_first_live(infx_index* idx, uint32_t total, const int32_t* first);
/* groups (distinct programs, counted ones included) and k_browse_scan launches of the last finalize that had browse queries */
int32_t infx_last_browse_stats(infx_stream* s, uint32_t* groups, uint32_t* launches);
/* FacetBuilder.BuildFacetsFromAllDocuments (Core/FacetBuilder.cs:110-181): for each of the ncol (<= INFX_MAX_FACET_COLS) uploaded columns cols[k] in
 * turn, the number of documents of the WHOLE corpus that are not Deleted per distinct value — counts_out holds sum(num_values) words, column k's
 * behind those of the columns before it.  One pass over the documents for all columns, synchronous.  The host drops null / empty values, orders and cuts. */
int32_t infx_facets_all(infx_stream* s, uint32_t ncol, const uint32_t* cols, uint32_t* counts_out);
/* Facets of the documents a filter accepts (not in the reference: the facet side of a pre-filter).  For each of the k (<= INFX_MAX_PREFILTERS) programs
 * progs[i] and each of the ncol (<= INFX_MAX_FACET_COLS) uploaded columns cols[c]: the number of documents of the WHOLE corpus that are not Deleted (the index's
 * real flags, never a per-query mask) and whose OWN column values the program accepts, per distinct value.  counts_out holds k x sum(num_values) words,
 * program-major: program i's block is laid out as infx_facets_all's; totals_out[i] = the documents program i accepts (= the count infx_filter_masks reports for
 * it).  ONE pass over the columns evaluates all k programs and counts every column (k_facets_filtered); it is split into several launches only when
 * the per-workgroup counters of the columns with few values would not fit in LDS for all k programs at once.  Works on a sharded index as infx_facets_all does
 * (every rank holds the whole columns and the global Deleted flags).  Synchronous.  ncol = 0 gives the totals alone.
 * infx_last_facets_filtered_stats: programs counted and k_facets_filtered launches of the stream's last call. */
int32_t infx_facets_filtered(infx_stream* s, uint32_t k, const infx_filter_prog* progs, uint32_t ncol, const uint32_t* cols,
                             uint32_t* counts_out /* k x sum(num_values), program-major */, uint32_t* totals_out /* k */);
int32_t infx_last_facets_filtered_stats(infx_stream* s, uint32_t* programs, uint32_t* launches);
/* ---- list columns: multi-valued document fields (Field.IsArray; kernels in csrc/list_columns.hip.inc) -------------------------------------------------
 * A list column is a CSR pair on the device, beside the scalar columns and outside their FILT_MAXCOL slots: elem_off[total_docs + 1] (uint32, ascending from
 * 0: a column holds fewer than 2^32 elements) and elem_codes[elem_off[total_docs]], the dictionary codes (< num_values) of the elements in document order.
 * infx_upload_list_column uploads (or replaces) list column lcol < INFX_MAX_LIST_COLS; total_docs = 0 drops it.  Exclusive call, as infx_upload_column.
 * Not on a sharded index (INFX_EUNSUPPORTED).
 * infx_list_leaf_build lowers k (<= INFX_LIST_LEAF_MAX) filter leaves over list column lcol to derived scalar columns in ONE k_list_leaf launch: slots[i] <
 * FILT_MAXCOL (64), distinct, names the scalar column slot that receives leaf i's column — uint32 per document, 1 where the leaf holds for at least one element
 * of the document's list, or, for an empty list, bit i of empty_bits; the slot then is an uploaded column of 2 values that a filter program reads like any
 * other.  maps: the leaves' bitmaps over the list column's codes side by side, word w of leaf i at maps[w * k + i], ceil(num_values / 32) * k words; they are
 * staged in LDS while that is at most INFX_LIST_LEAF_LDS_WORDS words and read from global memory beyond.  Synchronous: the columns are complete on return.
 * infx_list_facets counts, for each of k (<= INFX_MAX_PREFILTERS) accept sets, the element occurrences of every value of list column lcol among the accepted
 * documents, in ONE k_list_facets launch: masks[i] = document flags on the device, one byte per document, 0 = accepted (a mask slot of this stream, built by
 * infx_filter_masks: not Deleted and accepted) or NULL = every document that is not Deleted (the index's real flags).  counts_out: k x num_values words,
 * set-major.  Duplicates in a list count every time.  Synchronous. */
#define INFX_MAX_LIST_COLS 8
#define INFX_LIST_LEAF_MAX 16
#define INFX_LIST_LEAF_LDS_WORDS 2048
int32_t infx_upload_list_column(infx_index* idx, uint32_t lcol, uint32_t total_docs, const uint32_t* elem_off, const uint32_t* elem_codes, uint32_t num_values);
int32_t infx_list_leaf_build(infx_index* idx, uint32_t lcol, uint32_t k, const uint32_t* slots, const uint32_t* maps, uint32_t empty_bits);
int32_t infx_list_facets(infx_stream* s, uint32_t lcol, uint32_t k, const uint8_t* const* masks, uint32_t* counts_out);
/* A page of a document set in the order of a column (not in the reference: the order and the paging are this project's; DESIGN.md "list_documents").
 * Request i: the SET is the documents whose byte in `mask` is 0 — a mask slot of this stream (infx_stream_mask_slot, built by infx_filter_masks: not
 * Deleted and accepted) — or, mask = NULL, every document that is not Deleted (the index's real flags).  The KEY of a document is 1 + rank[its code] of
 * uploaded column `col` (infx_upload_sort_rank), or num_values + 1 - that when `ascending` is 0; col = -1: a constant.  The ORDER is (key, global internal
 * id) ascending — ties go by ascending id in both directions — a total order.  The answer is the rows at positions [offset, min(offset + limit, total))
 * of it, total = the size of the set: per row the DocumentKey, the global internal id and the column's code (0 without a column), in
 * keys_out / docs_out / codes_out at [i * INFX_POST_MAX_ROWS ..]; counts_out[i] rows, totals_out[i] = total; the rows from counts_out[i] up to limit read
 * -1 / -1 / 0, the ones beyond limit are not written.  offset >= total: no rows, no error.
 * 1 <= limit <= INFX_POST_MAX_ROWS whatever the index's post rows; offset < 2^31 (the kernels launched do not depend on it); digit_bits 4 .. 11 (11 in production: the width of a radix digit);
 * at most INFX_MAX_PREFILTERS requests (INFX_ECAPACITY).  No document is sorted: a radix select over the keys (ceil(bits(num_values + 1) / digit_bits)
 * histogram passes, at most three at 11 bits) finds the keys at both ends of the page, an ordered count / prefix / gather collects its <= 1024 rows and one
 * workgroup sorts those.  A mask build staged with infx_filter_masks is enqueued first, as ONE launch; nothing waits for the host between the kernels.
 * Exact and deterministic: the same bytes from any stream and grid.  Works on a sharded index (whole columns and global flags on every rank; the masks
 * of a sharded index serve this call only).  Synchronous.
 * infx_last_list_stats: histogram passes (summed over the requests) and kernel launches (the mask build included) of the stream's last call. */
typedef struct infx_list_req { const uint8_t* mask; int32_t col; int32_t ascending; uint32_t offset; uint32_t limit; uint32_t digit_bits; uint32_t reserved; } infx_list_req;
int32_t infx_list_ordered(infx_stream* s, uint32_t nreq, const infx_list_req* reqs, int64_t* keys_out, int32_t* docs_out, uint32_t* codes_out,
                          uint32_t* counts_out /* nreq */, uint32_t* totals_out /* nreq */);
int32_t infx_last_list_stats(infx_stream* s, uint32_t* hist_passes, uint32_t* launches);
/* Range facets of a document set over a numeric column (not in the reference: the buckets are this project's; DESIGN.md "range_facets").
 * Request i: the SET is the documents whose byte in `mask` is 0 — a mask slot of this stream (infx_stream_mask_slot, built by infx_filter_masks: not
 * Deleted and accepted) — or, mask = NULL, every document that is not Deleted (the index's real flags).  The work is on the dense sort rank of uploaded
 * column `col` (infx_upload_sort_rank), never on values: the caller turns its nedges (2 .. INFX_RANGE_MAX_EDGES) strictly increasing edges e_0 < .. < e_B
 * into thr[j] = the number of distinct ranks whose value compares < e_j (non-decreasing; a NaN ranks lowest and is counted under every edge), and
 * nan_ranks = 1 when the column's value of rank 0 is a NaN, else 0 (nan_ranks <= thr[j] <= num_values).  A document of rank r is counted in
 * counts_out[i * INFX_RANGE_SLOTS + k]: k = B + 2 (NaN) when r < nan_ranks, else k = #{j : thr[j] <= r} — k = 0 below e_0, k = 1 .. B the half-open
 * bucket [e_(k-1), e_k), k = B + 1 at or above e_B; B + 3 words are written per request, their sum is the size of the set.  min_rank_out[i] /
 * max_rank_out[i]: the smallest and largest rank >= nan_ranks in the set; min_rank_out[i] = 0xFFFFFFFF when there is none (max_rank_out[i] is 0 then).
 * At most 16 requests (INFX_ECAPACITY), all counted by ONE k_range_counts launch that walks the corpus once: the requests are taken in the order
 * (mask, col), so the ones that share a mask read its bytes once and the ones that share a column too read the codes and ranks once.  A mask build
 * staged with infx_filter_masks is enqueued first, as ONE launch.  Integer atomics only, none decides a position: the same bytes from any stream
 * and grid.  Works on a sharded index (whole columns and global flags on every rank; masks by global id).  Synchronous.
 * infx_last_range_stats: requests and k_range_counts launches (0 or 1) of the stream's last call. */
#define INFX_RANGE_MAX_EDGES 257
#define INFX_RANGE_SLOTS 260
typedef struct infx_range_req { const uint8_t* mask; int32_t col; uint32_t nedges; uint32_t nan_ranks; uint32_t reserved; const uint32_t* thr; } infx_range_req;
int32_t infx_range_counts(infx_stream* s, uint32_t nreq, const infx_range_req* reqs, uint32_t* counts_out /* nreq x INFX_RANGE_SLOTS */,
                          uint32_t* min_rank_out /* nreq */, uint32_t* max_rank_out /* nreq */);
int32_t infx_last_range_stats(infx_stream* s, uint32_t* requests, uint32_t* launches);
/* Field statistics of a document set over a numeric column, whole or per value of a second column (not in the reference: the aggregate is this
 * project's; DESIGN.md "field_stats").
 * infx_upload_column_values: the raw values of column col's codes — bits[v] the 8 bytes of distinct value v: an int64 (kind 1) or the bit pattern of a
 * double (kind 2) — with the scale they are summed at: scale_exp the lowest exponent of a set mantissa bit over the finite values that are not zero
 * (0 for kind 1 and for a column without such a value), nlimbs = ceil((1 + highest exponent of a set bit - scale_exp) / 32), at least 1, at most 4 (kind 1:
 * at most 2).  Both are checked against the values (INFX_EINVAL).  8 B per distinct value: the limbs are cut from the value on the device by integer
 * shifts, so a member costs one 8 B gather, not 16 B of precomputed limbs.  Exclusive call, like infx_upload_sort_rank; a re-upload of the column voids the
 * table as it voids the sort rank.
 * infx_field_stats, request i: the SET is the documents whose byte in `mask` is 0 — a mask slot of this stream — or, mask = NULL, every document that is
 * not Deleted.  `col` needs its sort rank (infx_upload_sort_rank) and its value table; `group_col` is any uploaded column of at most
 * INFX_STATS_MAX_GROUPS distinct values, or -1.  The request has one SLOT per distinct value of group_col (in code order), one in all without it; the
 * slots of request i follow those of request i - 1 in slots_out.  A member document adds to the slot of its group code: one of four counters by the class
 * of its value (finite, NaN, +inf, -inf), its sort rank to min_rank / max_rank unless it is a NaN (min_rank = 0xFFFFFFFF and max_rank = 0: the slot saw no
 * such value), and, when finite, the nlimbs unsigned 32-bit digits of |v| / 2^scale_exp, with the sign of v, to the signed 64-bit sums sum[0 .. nlimbs)
 * (the others are 0).  The exact sum of the slot's finite values is 2^scale_exp * (sum[0] + sum[1] * 2^32 + ..); with fewer than 2^31 documents no sum
 * overflows.  Every accumulation is an integer atomic — no floating-point add, no order: the same bytes from any stream, grid and placement.
 * At most 16 requests (INFX_ECAPACITY), all answered by ONE k_field_stats launch that walks the corpus once: the requests are taken in the order
 * (mask, col, group_col), so the ones that share a mask read its bytes once and the ones that share a value column too read its codes, values and ranks
 * once.  A request's slots lie in LDS while they fit (requests in ascending size, 16 384 words per workgroup), else in global memory.  A mask build
 * staged with infx_filter_masks is enqueued first, as ONE launch.  Works on a sharded index.  Synchronous.
 * infx_last_field_stats_info: requests and k_field_stats launches (0 or 1) of the stream's last call. */
#define INFX_STATS_MAX_GROUPS 4096
#define INFX_STATS_MAX_LIMBS 4
typedef struct infx_stats_req { const uint8_t* mask; int32_t col; int32_t group_col; } infx_stats_req;
typedef struct infx_stats_slot { uint32_t finite; uint32_t nan; uint32_t pinf; uint32_t ninf; uint32_t min_rank; uint32_t max_rank; int64_t sum[INFX_STATS_MAX_LIMBS]; } infx_stats_slot;
int32_t infx_upload_column_values(infx_index* idx, uint32_t col, uint32_t num_values, const uint64_t* bits, int32_t kind, int32_t scale_exp, uint32_t nlimbs);
int32_t infx_field_stats(infx_stream* s, uint32_t nreq, const infx_stats_req* reqs, infx_stats_slot* slots_out /* sum of the requests' slots */);
int32_t infx_last_field_stats_info(infx_stream* s, uint32_t* requests, uint32_t* launches);
/* Field statistics of a document set per RANGE BUCKET of a second numeric column (not in the reference: the aggregate is this project's; DESIGN.md
 * "bucket_stats").
 * Request i: the SET is infx_field_stats' — the documents whose byte in `mask` is 0 (a mask slot of this stream), or, mask = NULL, every document that is not
 * Deleted.  `col` is the summed column, with its sort rank and its value table uploaded as for infx_field_stats; `bucket_col` is the column the buckets cut,
 * with its sort rank uploaded; nedges, thr and nan_ranks are infx_range_counts' over bucket_col (2 .. INFX_RANGE_MAX_EDGES thresholds, non-decreasing,
 * nan_ranks <= thr[j] <= bucket_col's num_values; nan_ranks 0 or 1); reserved is 0.  col == bucket_col is allowed.  The request has B + 3 = nedges + 2 SLOTS
 * in infx_range_counts' order of counters — slot 0 below e_0, 1 .. B the half-open buckets, B + 1 at or above e_B, B + 2 the members whose bucket_col value is
 * a NaN — and the slots of request i follow those of request i - 1 in slots_out.  A member document of bucket rank r adds to slot k (k = B + 2 when
 * r < nan_ranks, else k = #{j : thr[j] <= r}) exactly what infx_field_stats adds to the slot of a group code: one of four counters by the class of its
 * VALUE, the value's sort rank to min_rank / max_rank unless it is a NaN, its limbs to the signed sums.  finite + nan + pinf + ninf of slot k is what
 * infx_range_counts counts in counter k.  Every accumulation is an integer atomic — no floating-point add, no order: the same bytes from any stream, grid
 * and placement.
 * At most 16 requests (INFX_ECAPACITY), all answered by ONE k_bucket_stats launch that walks the corpus once: the requests are taken in the order
 * (mask, col, bucket_col), so the ones that share a mask read its bytes once and the ones that share a value column too read its codes, values and ranks
 * once.  Every request's thresholds lie in LDS; its slots lie there too while they fit (infx_field_stats' rule and its two launch shapes, each budget less
 * the thresholds), else in global memory.  A mask build staged with infx_filter_masks is enqueued first, as ONE launch.  Works on a sharded index.
 * Synchronous.
 * infx_last_bucket_stats_info: requests and k_bucket_stats launches (0 or 1) of the stream's last call, and its requests whose slots lay in a workgroup's
 * LDS (256 threads), in a CU's whole LDS (1024 threads) and in global memory. */
typedef struct infx_bucket_stats_req { const uint8_t* mask; int32_t col; int32_t bucket_col; uint32_t nedges; uint32_t nan_ranks; uint32_t reserved; const uint32_t* thr; } infx_bucket_stats_req;
int32_t infx_bucket_stats(infx_stream* s, uint32_t nreq, const infx_bucket_stats_req* reqs, infx_stats_slot* slots_out /* sum of the requests' nedges + 2 */);
int32_t infx_last_bucket_stats_info(infx_stream* s, uint32_t* requests, uint32_t* launches, uint32_t* small_lds, uint32_t* big_lds, uint32_t* in_global);
/* Quantiles of a document set over a numeric column, whole and per value of a second column (not in the reference: the aggregate is this project's;
 * DESIGN.md "field_quantiles").
 * Request i: the SET is infx_field_stats': the documents whose byte in `mask` is 0 — a mask slot of this stream — or, mask = NULL, every document that is
 * not Deleted.  The work is on the dense sort rank of uploaded column `col` (infx_upload_sort_rank), never on values; nan_ranks = 1 when the column's
 * value of rank 0 is a NaN, else 0: a member whose rank is below it is counted as a NaN and is in no quantile.  `group_col` is any uploaded column of at
 * most INFX_STATS_MAX_GROUPS distinct values, or -1.  The request has one SLOT per distinct value of group_col (in code order) and, BEHIND them, one for the
 * whole set — that one alone without group_col; the slots of request i follow those of request i - 1 in slots_out: count = the slot's members that are
 * not NaNs, nan = the others.  ranks_out holds nq words per slot, in the same order: word t is the sort rank at 0-based position
 * floor((count - 1) * q[t]) of the slot's non-NaN members in ascending rank order — the product one IEEE double multiplication — or 0xFFFFFFFF when count
 * is 0.  1 <= nq <= INFX_QUANT_MAX, every q[t] in [0, 1] (no NaN), in any order, duplicates allowed.
 * No document is sorted: a radix select over the keys 1 + rank, most significant digit first, for ALL targets (slot, t) of ALL requests at once.  A pass is
 * ONE k_quant_hist launch — a walk over the corpus that takes the requests in the order (mask, col, group_col), so the ones that share a mask read its bytes
 * once and the ones that share a column too read its codes and ranks once — and ONE k_quant_pick launch, on the stream.  digit_bits: the width of a radix digit, 4 .. 11, or
 * 0: the call chooses — the widest at which the bins of one pass of the whole call take at most 64 MiB, per request narrowed to the least width of the same
 * number of passes, ceil(bits(num_values + 1) / width); a width given here is lowered to that bound too.  The width changes the number of passes, never the
 * answer.  Bins lie in LDS while they fit (as infx_field_stats' slots; a request's groups' bins and the whole set's are placed apart), else in global memory.  Integer atomics only, none decides a position:
 * the same bytes from any stream, grid, width and placement.  At most 16 requests (INFX_ECAPACITY).  A mask build staged with infx_filter_masks is
 * enqueued first, as ONE launch; nothing waits for the host between the kernels.  Works on a sharded index.  Synchronous.
 * infx_last_field_quantiles_info, of the stream's last call: requests, k_quant_hist launches (= passes), kernel launches (the mask build included), the
 * call's digit width, and how many (request, pass) pairs had their bins — the groups', without group_col the whole set's — in LDS / in global memory. */
#define INFX_QUANT_MAX 16
typedef struct infx_quant_req { const uint8_t* mask; int32_t col; int32_t group_col; uint32_t nq; uint32_t digit_bits; uint32_t nan_ranks; uint32_t reserved; double q[INFX_QUANT_MAX]; } infx_quant_req;
typedef struct infx_quant_slot { uint32_t count; uint32_t nan; } infx_quant_slot;
int32_t infx_field_quantiles(infx_stream* s, uint32_t nreq, const infx_quant_req* reqs, infx_quant_slot* slots_out /* sum of the requests' slots */,
                             uint32_t* ranks_out /* sum of the requests' slots x nq */);
int32_t infx_last_field_quantiles_info(infx_stream* s, uint32_t* requests, uint32_t* hist_passes, uint32_t* launches, uint32_t* digit_bits, uint32_t* lds_rows, uint32_t* global_rows);
/* A page of the HEADS of a document set's groups, in the order of a column, with the groups' sizes (not in the reference: the collapsed listing is this
 * project's; DESIGN.md "list_groups").
 * Request i: the SET, the KEY and the ORDER (key, global internal id) are infx_list_ordered's, over `mask` (a mask slot of this stream, or NULL: every
 * document that is not Deleted), column `col` (-1: a constant key) and `ascending`.  A GROUP is one code of uploaded column `group_col` (any kind, any
 * number of values; it may be `col`); the HEAD of a group with a member is its member that comes first in the ORDER.  The answer is the rows at positions
 * [offset, min(offset + limit, groups)) of the heads in the ORDER — infx_list_ordered over the SET restricted to the heads: per row the DocumentKey, the
 * global internal id, the code of `col` (0 without a column), the group's code and the number of members of that group in the SET, in keys_out / docs_out /
 * codes_out / gcodes_out / sizes_out at [i * INFX_POST_MAX_ROWS ..]; counts_out[i] rows, group_totals_out[i] = the number of groups with a member (the exact
 * distinct count of group_col over the set), totals_out[i] = the size of the SET.  Rows from counts_out[i] up to limit read -1 / -1 / 0 / 0 / 0.
 * offset >= groups: no rows, no error.  limit, offset, digit_bits and the number of requests as in infx_list_ordered.
 * A SPEC is (mask, group_col, col, ascending); the requests of a call are taken in spec order and the specs run one after another on the stream:
 *   k_group_heads       one walk over the corpus per spec: every member takes the 64-bit minimum of (key << 32 | id) into the entry of its group code in the
 *                       head table (8 B per value of group_col), asked of the memory only when a plain read shows a larger entry.  Tables of at most 8 191
 *                       values lie in LDS per workgroup, up to 20 479 values in the whole LDS of a CU under one workgroup of 1024 threads, and are merged
 *                       with one global minimum per entry that saw a member; larger tables are hit in global memory.  The walk also counts the set.
 *   k_group_heads_mask  byte d = 0 exactly when d is a member and the low word of its group's entry is d: the heads as a mask.
 *   the page            infx_list_ordered's select / count / prefix / gather / sort over the heads mask, per request.
 *   k_group_page, k_group_sizes   the group codes of every page's rows, sorted; ONE further walk over the SET for all requests of the spec looks every member's
 *                       code up among them and adds to the row's counter.
 * A minimum has no order and the adds are integer adds, none decides a position: the same bytes from any stream, grid and placement.  A mask build staged
 * with infx_filter_masks is enqueued first, as ONE launch; nothing waits for the host between the kernels.  Works on a sharded index (whole columns and
 * global flags on every rank).  Synchronous.
 * infx_last_group_list_stats: head passes (= specs), histogram passes (summed over the requests) and kernel launches (the mask build included) of the
 * stream's last call. */
typedef struct infx_group_list_req { const uint8_t* mask; int32_t col; int32_t ascending; uint32_t offset; uint32_t limit; uint32_t digit_bits; uint32_t reserved; int32_t group_col; int32_t reserved2; } infx_group_list_req;
int32_t infx_list_grouped(infx_stream* s, uint32_t nreq, const infx_group_list_req* reqs, int64_t* keys_out, int32_t* docs_out, uint32_t* codes_out,
                          uint32_t* gcodes_out, uint32_t* sizes_out, uint32_t* counts_out /* nreq */, uint32_t* group_totals_out /* nreq */,
                          uint32_t* totals_out /* nreq */);
int32_t infx_last_group_list_stats(infx_stream* s, uint32_t* head_passes, uint32_t* hist_passes, uint32_t* launches);
/* infx_list_grouped's page with the first `per_group` MEMBERS of every listed group (not in the reference; DESIGN.md "list_group_members").
 * Request i is infx_list_grouped's, field for field, plus per_group: 1 .. INFX_GROUP_MEMBERS_MAX_PER_GROUP (16), and limit * per_group <=
 * INFX_GROUP_MEMBERS_MAX (4096).  The rows, their group codes, sizes and the three totals are exactly infx_list_grouped's of the same request, in rows_out
 * (the heads' global internal ids) / gcodes_out / sizes_out at [i * INFX_POST_MAX_ROWS ..] and counts_out / group_totals_out / totals_out at [i].  The members
 * of row r are the first min(per_group, size) members of its group in the ORDER (key, global internal id), the head first: per (row r, place p) the
 * DocumentKey, the global internal id and the code of `col` (0 without a column) in member_keys_out / member_docs_out / member_codes_out at
 * [i * INFX_GROUP_MEMBERS_MAX + r * per_group + p]; places without a member, and every place of the rows from counts_out[i] up to limit, read -1 / -1 / 0.
 * member_counts_out[i * INFX_POST_MAX_ROWS + r]: the places of row r that hold a member.
 * The front half is infx_list_grouped's: k_group_heads, k_group_heads_mask, the page, k_group_page.  Then, per spec:
 *   k_group_members      takes k_group_sizes' place, one walk over the SET for as many consecutive requests of the spec as fit the whole LDS of a CU together
 *                        (per request 2 * limit + 2 * limit * per_group words: one always fits a workgroup's): a member whose group code is among the page's
 *                        adds to the row's LDS counter and enters (key << 32 | id) into the row's per_group LDS slots, which keep the smallest composites in
 *                        ascending order under any interleaving (group_members.h); the LDS slots then enter the row's global slots the same way.
 *   k_group_member_rows  the slots as documents, keys and codes.
 * Minima and integer adds only: the same bytes from any stream, grid, placement and packing.  Works on a sharded index.  Synchronous.
 * infx_last_group_members_stats: head passes (= specs), histogram passes, member walks (k_group_members launches) and kernel launches (the mask build
 * included) of the stream's last call. */
#define INFX_GROUP_MEMBERS_MAX_PER_GROUP 16
#define INFX_GROUP_MEMBERS_MAX 4096      /* limit * per_group of a request */
typedef struct infx_group_members_req { const uint8_t* mask; int32_t col; int32_t ascending; uint32_t offset; uint32_t limit; uint32_t digit_bits; uint32_t reserved; int32_t group_col; int32_t reserved2; uint32_t per_group; uint32_t reserved3; } infx_group_members_req;
int32_t infx_list_group_members(infx_stream* s, uint32_t nreq, const infx_group_members_req* reqs, int32_t* rows_out, uint32_t* gcodes_out, uint32_t* sizes_out,
                                uint32_t* member_counts_out, int64_t* member_keys_out, int32_t* member_docs_out, uint32_t* member_codes_out,
                                uint32_t* counts_out /* nreq */, uint32_t* group_totals_out /* nreq */, uint32_t* totals_out /* nreq */);
int32_t infx_last_group_members_stats(infx_stream* s, uint32_t* head_passes, uint32_t* hist_passes, uint32_t* member_walks, uint32_t* launches);
/* A page of a document set's GROUPS ranked by a figure of the group (not in the reference: the ranking is this project's; DESIGN.md "top_groups").
 * Request i: the SET is infx_field_stats' — the documents whose byte in `mask` is 0 (a mask slot of this stream), or, mask = NULL, every document that is not
 * Deleted.  A GROUP is one code of uploaded column `group_col`: any kind, ANY number of values, its facet tie order uploaded with infx_upload_group_rank (a
 * permutation of the codes; a column re-upload voids it).  `col` is a value column with its sort rank and value table uploaded as for infx_field_stats, or
 * -1, which allows by = INFX_TOP_BY_SIZE only.  The FIGURE of a group is, by `by`: its members in the SET (SIZE), those whose value is not a NaN (COUNT),
 * the smallest / largest sort rank of those (MIN / MAX), the exact sum (SUM: an int column's 128-bit integer, a double column's real sum rounded once, as a
 * double), the exact mean rounded once (MEAN).  A group whose figure is none (MIN / MAX / MEAN without a value that is not a NaN) or a NaN (+inf and -inf
 * among its members) has NO figure.  ORDER: the groups with a member and a figure by the figure, ascending or descending, then the groups with a member and
 * no figure, in both directions; every tie by the group rank, ascending in both directions.  The answer is the rows [offset, min(offset + limit, groups)):
 * per row the group's code and its slot — infx_field_stats' slot of that group; without a value column `finite` holds the members, min_rank is all ones and
 * the rest zero — in codes_out / slots_out at [i * INFX_POST_MAX_ROWS ..]; counts_out[i] rows, group_totals_out[i] the groups with a member,
 * totals_out[i] the size of the SET.  offset >= groups: no rows, no error.  limit, offset, digit_bits and the number of requests as in infx_list_ordered.
 * A TABLE is (mask, col, group_col); the requests of a call are taken in table order and the tables run one after another on the stream:
 *   accumulate     one walk per table: k_field_stats with the table as its one request (infx_field_stats' slots and placement: a workgroup's LDS, a CU's
 *                  whole LDS under 1024 threads, else global atomics; no cap on the slots), or k_top_sizes (one member counter per code) without a column
 *   k_top_keys     per request and code the composite [class | figure | group rank] of top_select.h; counts the groups with a member and the SET
 *   k_top_hist / k_top_pick   radix select over the composites, most significant digit first, for positions offset and offset + rows - 1 at once; the
 *                  requests of a table advance in the same launches, each for the passes its figure's width needs
 *   k_top_gather / k_top_page   the codes between the two composites found (composites are distinct: exactly the page), sorted in LDS, with their slots
 * Integer adds, minima and maxima only, none decides an answer's bytes: the same bytes from any stream, grid and placement.  A mask build staged with
 * infx_filter_masks is enqueued first, as ONE launch; one copy brings all pages back.  Works on a sharded index.  Synchronous.
 * infx_last_top_groups_info: requests, accumulate passes (= tables walked), select passes (k_top_hist launches), kernel launches (the mask build
 * included), and the tables accumulated in a workgroup's LDS / a CU's whole LDS / global memory of the stream's last call. */
#define INFX_TOP_BY_SIZE 0
#define INFX_TOP_BY_COUNT 1
#define INFX_TOP_BY_MIN 2
#define INFX_TOP_BY_MAX 3
#define INFX_TOP_BY_SUM 4
#define INFX_TOP_BY_MEAN 5
typedef struct infx_top_req { const uint8_t* mask; int32_t col; int32_t group_col; uint32_t by; int32_t ascending; uint32_t offset; uint32_t limit; uint32_t digit_bits; uint32_t reserved; } infx_top_req;
int32_t infx_upload_group_rank(infx_index* ix, uint32_t col, uint32_t num_values, const uint32_t* rank);
int32_t infx_top_groups(infx_stream* s, uint32_t nreq, const infx_top_req* reqs, uint32_t* codes_out, infx_stats_slot* slots_out, uint32_t* counts_out /* nreq */,
                        uint32_t* group_totals_out /* nreq */, uint32_t* totals_out /* nreq */);
int32_t infx_last_top_groups_info(infx_stream* s, uint32_t* requests, uint32_t* accumulate_passes, uint32_t* select_passes, uint32_t* launches,
                                  uint32_t* small_lds, uint32_t* big_lds, uint32_t* in_global);
/* The exact number of distinct codes of a column over a document set, whole and per group (not in the reference: DESIGN.md "field_distinct").
 * Request i: the SET is infx_field_stats' — the documents whose byte in `mask` is 0 (a mask slot of this stream), or, mask = NULL, every document that is not
 * Deleted.  `col` is any uploaded column (no sort rank or value table needed), `group_col` any uploaded column of at most INFX_STATS_MAX_GROUPS values, or
 * -1.  A member's PAIR is (its code in group_col, 0 without one; its code in col).  distinct_out[i]: the codes of col among the members; totals_out[i]: the
 * members; with a group column, by group code at [i * INFX_STATS_MAX_GROUPS ..]: group_sizes_out the members of the group, group_distinct_out the codes of
 * col among them (without one those entries are not written).
 * A SPEC is (mask, col, group_col, placement); the requests of a call are taken in spec order, each spec is marked in ONE set walk and the specs run one after
 * another on the stream, in one workspace.  G = the group column's values (1 without), V = col's:
 *   1 LDS      G rows of V bits (rows padded to 32-bit words) and G size counters in a workgroup's LDS, by k_field_stats' two budgets; merged once
 *   2 bitmap   the rows in global memory, at most 2^32 bits: a member's atomicOr only where a plain read shows its bit clear; sizes in LDS
 *   3 hash     an open-addressing set of 64-bit keys (pair index + 1), capacity the power of two >= 2 x min(documents, G x V): it cannot fill.  A probe
 *              visits at most `capacity` slots, then raises a flag that fails the call (INFX_ECAPACITY); installs are counted per group in LDS; with more
 *              than one group a V-bit side row gives the whole set's count
 *   k_distinct_count   popcounts the rows of placements 1 and 2 per group; k_distinct_union ORs them into a union row, whose popcount is the whole set's count
 * placement 0: LDS when it fits, else the smaller of bitmap and hash workspace.  1 / 2 / 3 force one; one that does not fit falls to the next larger.
 * Bit ORs, compare-and-swap installs counted once and integer adds only: the same bytes from any stream, grid and placement.  A mask build staged with
 * infx_filter_masks is enqueued first, as ONE launch; one copy brings all counters back.  Works on a sharded index.  Synchronous.
 * infx_last_field_distinct_info: requests, kernel launches (the mask build included), and the specs marked in LDS / a global bitmap / a hash set of the
 * stream's last call. */
typedef struct infx_distinct_req { const uint8_t* mask; int32_t col; int32_t group_col; uint32_t placement; uint32_t reserved; } infx_distinct_req;
int32_t infx_field_distinct(infx_stream* s, uint32_t nreq, const infx_distinct_req* reqs, uint32_t* distinct_out /* nreq */, uint32_t* totals_out /* nreq */,
                            uint32_t* group_sizes_out /* nreq x INFX_STATS_MAX_GROUPS */, uint32_t* group_distinct_out /* nreq x INFX_STATS_MAX_GROUPS */);
int32_t infx_last_field_distinct_info(infx_stream* s, uint32_t* requests, uint32_t* launches, uint32_t* lds_passes, uint32_t* bitmap_passes, uint32_t* hash_passes);

/* ---- measurement hooks (bench.py) ------------------------------------------------------------------------------ */
/* Durations (ms) of the last Stage-1 accumulate / select / Stage-2 launches on this stream, from HIP events recorded on
 * the stream the kernels ran on. */
/* ---- Whole batch on the device (unsharded index) -----------------------------------------------------------------
 * infx_search_fused runs SearchEngine.Search for a batch with ONE host synchronisation: accumulate -> tier rules -> select ->
 * coverage-stage candidate assembly (SearchPipeline.ExecuteCoverageStage, SearchPipeline.cs:330-420, incl. the WordMatcher
 * overlap / first-unique lookups of WordMatcher.Lookup, WordMatcher.cs:95-186) -> Stage 2 -> TopKHeap + ConsolidateSegments +
 * CalculateTruncationIndex (SearchPipeline.cs:422-560); only max_results rows per query return to the host.
 * The host supplies what needs the dictionaries: query terms / idf / roles (as for infx_stage1_accumulate), the prepared
 * coverage query, and per query the WordMatcher doc-id lists as ranges of the uploaded arrays. */
int32_t infx_upload_wordmatcher(infx_index* idx, uint64_t n_exact, const int32_t* exact_docs, uint64_t n_ld1, const int32_t* ld1_docs);

typedef struct infx_wm_list {      /* one ascending doc-id list */
    uint32_t src;                  /* 0: exact_docs, 1: ld1_docs (infx_upload_wordmatcher), 2: the call's `owned` buffer (affix matches) */
    uint32_t len;
    uint64_t off;
} infx_wm_list;

/* ---- Dictionary lookups of query planning on the device ------------------------------------------------------------
 * The reference resolves a query word to doc-id lists through three host dictionaries; uploaded once, the lookups run on the GPU:
 *   - WordMatcher.Lookup (WordMatcher/WordMatcher.cs:201-246): the word in the exact-word dictionary; for words of min_ld1..max_ld1 characters the word
 *     and each of its single-character deletions in the symmetric-delete dictionary and the exact dictionary;
 *   - WordMatcher.LookupAffix (:277-354): the words the query word is a prefix of, then those it is a suffix of — at most 4096 trie terms in that
 *     order — each contributing the LAST document that contains it (quirk Q13);
 *   - FstIndex.MatchWithinEditDistance1 (Indexing/Fst/FstIndex.cs:202-351): index terms with a suffix within Levenshtein distance 1 of the word.
 * Keys are UTF-16 strings in one arena per dictionary (key k = chars[key_offs[k] .. key_offs[k+1])); the library builds its own hash tables.
 * exact/ld1 list_offs index the doc-id arrays handed to infx_upload_wordmatcher (call that first).  affix_fwd / affix_rev: ids of the words of at
 * least min_ld1 characters, in ordinal order of the word / of the reversed word (the order the reference's trie walk meets them in). */
int32_t infx_upload_wm_dictionary(infx_index* idx,
                                  uint32_t n_exact_keys, const uint32_t* exact_key_offs /* n+1 */, const uint16_t* exact_chars, const uint64_t* exact_list_offs /* n+1 */,
                                  uint32_t n_ld1_keys, const uint32_t* ld1_key_offs, const uint16_t* ld1_chars, const uint64_t* ld1_list_offs,
                                  uint32_t n_words, const uint32_t* word_offs /* n+1 */, const uint16_t* word_chars, const int32_t* word_last_doc,
                                  uint32_t n_affix, const uint32_t* affix_fwd, const uint32_t* affix_rev, int32_t min_ld1, int32_t max_ld1);
/* Trie of the REVERSED index terms as CSR (node 0 = root; children of node v = edges edge_start[v] .. edge_start[v+1), ascending label), node_term[v] =
 * term id ending at v or -1; sorted_terms = all term ids in ordinal order of their text (FstIndex returns matches in that order). */
int32_t infx_upload_term_trie(infx_index* idx, uint32_t n_nodes, const uint32_t* edge_start /* n_nodes+1 */, const uint16_t* edge_label, const uint32_t* edge_child,
                              const int32_t* node_term, uint32_t n_terms, const uint32_t* sorted_terms);
/* FstIndex.MatchWithinEditDistance1 for a batch of words (word w = chars[word_offs[w] .. word_offs[w+1])): counts_out[w] = number of matching terms,
 * members_out[w*cap ..] = the first min(count, cap) of them in ordinal order (the reference keeps the first 1024, VectorModel.cs:660).
 * status_out[w]: 0 ok; 1 the walk outgrew the kernel's work lists (very short words fan out over the whole vocabulary) and 2 word length outside 1..64
 * (the reference switches to another walk, FstIndex.cs:362-440) — in both cases nothing was written for w and the caller expands it on the host. */
int32_t infx_ld1_expand(infx_stream* s, uint32_t nwords, const uint32_t* word_offs /* n+1 */, const uint16_t* chars, uint32_t cap,
                        int32_t* members_out /* nwords x cap */, uint32_t* counts_out, uint32_t* status_out);
/* infx_union_build with the expansion fused in: union v takes its members from members[member_offs[v] .. member_offs[v+1]) when word_of[v] < 0, or from the LD1
 * expansion of word word_of[v] (each word at most once; its member range must be empty).  k_ld1 closes the word unions' member ranges on the device and the union
 * kernels follow on the same stream: ONE wait for the device per batch (the counts) instead of two.  A word the kernel hands back (status != 0) yields an empty
 * union: expand it on the host and build again.  The expansions come back as from infx_ld1_expand. */
int32_t infx_union_build_ld1(infx_stream* s, uint32_t nv, const uint32_t* member_offs, const int32_t* members, const int32_t* word_of /* nv */,
                             uint32_t nwords, const uint32_t* word_offs /* n+1 */, const uint16_t* chars, uint32_t cap,
                             uint32_t* counts_out /* nv */, int32_t* ld1_members_out /* nwords x cap */, uint32_t* ld1_counts_out, uint32_t* ld1_status_out);
/* WordMatcher lists of ONE coverage query as the device produces them (parity tests): lists_out[INFX_MAX_WM_LISTS], *nlists_out of them; src 2 offsets
 * index owned_out (owned_cap ints, >= 4096 per word of the query). */
int32_t infx_wm_lookup_debug(infx_stream* s, const infx_cov_query* cq, infx_wm_list* lists_out, uint32_t* nlists_out, int32_t* owned_out, uint64_t owned_cap);

#define INFX_FQ_SKIP 1u            /* blank / unsupported query text: empty result */
#define INFX_FQ_SHORT 2u           /* 1..3 characters without delimiter (SearchPipeline.cs:108-120) */
#define INFX_FQ_SHORTSKIP 4u       /* short query whose prefix population exceeds 500: coverage is skipped */
#define INFX_FQ_COV 8u             /* coverage enabled (engine setup && Query.EnableCoverage) */
#define INFX_FQ_UNSUPPORTED 16u    /* result flag bit0 is set */
#define INFX_FQ_BROWSE 64u         /* with INFX_FQ_SKIP: empty text + EnableFacets — the first max_results live documents the query's filter accepts (browse rows, above) */
#define INFX_FQ_WMDEV 32u          /* the WordMatcher lists of this query are looked up on the device (infx_upload_wm_dictionary) from the words of its
                                      infx_cov_query; wm_off / wm_count are ignored (leave wm_count 0).  Admissible while words x (3 + 2*max_ld1) <= INFX_MAX_WM_LISTS */
#define INFX_MAX_WM_LISTS 256
typedef struct infx_fused_query {
    int32_t  dev;                  /* index into q[] of the Stage-1 part, or -1 (no index term) */
    uint32_t flags;                /* INFX_FQ_* */
    uint32_t wm_off, wm_count;     /* lists[wm_off .. +wm_count), non-empty lists only, <= INFX_MAX_WM_LISTS */
    int32_t  max_results;          /* Query.MaxNumberOfRecordsToReturn */
    int32_t  reserved;             /* set by the library */
} infx_fused_query;

/* nd Stage-1 queries q[] (+ terms), nq search queries fq[]/cq[] (nq >= nd; cq[i] is ignored unless coverage runs for i).
 * All queries must share one depth.  out_*: nq x max_results rows; out_flags bits as infx_engine_search_batch. */
int32_t infx_search_fused(infx_stream* s, uint32_t nd, const infx_query* q, uint32_t nterms, const infx_term* terms,
                          uint32_t nq, const infx_fused_query* fq, const infx_cov_query* cq,
                          uint32_t nlists, const infx_wm_list* lists, uint32_t owned_n, const int32_t* owned,
                          int32_t depth, int32_t max_results, int32_t want_debug,
                          int64_t* out_keys, float* out_scores, uint8_t* out_ties, uint32_t* out_counts, uint32_t* out_flags);
/* Document-sharded operation: the same device stages, cut where the collectives go. Rows carry GLOBAL internal ids.
 *   infx_stage1_accumulate (local) -> all-reduce(sum) of the class histograms
 *   infx_shard_select   : tier rules from the GLOBAL counts + local first-pass top-`depth` -> all-gather; infx_shard_replay_* (exact cut) -> all-gather of hits / hit counts (RCCL)
 *   infx_shard_stage2   : merge of the nshards lists, candidate assembly, Stage 2 on the rows whose document this shard holds
 *                         (all other rows are zero)                                  -> all-reduce(sum) of outs (nq x 2*depth x 12 B)
 *   infx_shard_finalize : final ordering / truncation from the merged rows (identical on every rank).
 * The exchange buffers (hits_out / hitcount_out, all_hits / all_hitcounts, outs_out, merged_outs) may be host OR device memory: device
 * pointers (e.g. the tensors a torch.distributed / RCCL collective works on) are copied device-to-device, nothing crosses PCIe.
 * Every shard needs the GLOBAL DocumentKey table (infx_upload_doc_keys_all) and the WordMatcher lists (global ids). */
int32_t infx_upload_doc_keys_all(infx_index* idx, uint32_t total_docs, const int64_t* keys);
int32_t infx_shard_select(infx_stream* s, uint32_t nd, const infx_counts* global_counts, int32_t depth, infx_hit* hits_out, uint32_t* hitcount_out,
                          float* next_out /* nd: best first-pass score this shard left out of its list (0: none); NULL = not wanted */);
/* The reference's Stage-1 cut across document shards, bit for bit (Bm25Scorer.cs:195-329 chunks, :350-368 MaxScore skips, :654-670 UpdateTopK on the
 * BCL heap): shards must begin at multiples of 65 536 documents (whole Roaring containers), so the reference's sequential walk is the shards' walks one
 * after the other, coupled only through the heap.  Between infx_shard_select and infx_shard_stage2:
 *   infx_shard_select (hits, counts, next)                                 -> all-gather of the three                                [Exchange 2a]
 *   infx_shard_replay_local : global ambiguity test (identical on every rank) + this shard's chunks: exact scores, candidates the heap could
 *                             still take, validity intervals of the MaxScore skips; *blob_bytes = size of the packed result
 *   infx_shard_replay_blob  : copies it to host or device memory             -> all-gather of the blobs, padded to the largest        [Exchange 2c]
 *   infx_shard_replay_merge : the OWNER of a flagged query (query mod nshards) replays UpdateTopK over shard 0's chunks, then shard 1's, ...;
 *                             hits_out / hitcount_out = this rank's contribution to the final lists: the exact list for owned flagged queries,
 *                             nothing for other flagged queries, the first-pass list otherwise                                      -> all-gather [Exchange 2b]
 *                             hitcount 0xFFFFFFFF: the owner could not certify the parallel replay (rare) -> infx_shard_replay_chain
 *   infx_shard_replay_chain : the literal sequential replay of the queries with need[q] != 0, continued from shard to shard: state = nd x (2 + 2*depth)
 *                             words {n, threshold bits, doc[depth], score bits[depth]} (heap array order), zero for shard 0; pass the output of shard r
 *                             to shard r+1; the last shard's state is the reference's final heap.  depth == infx_config.max_depth. */
int32_t infx_shard_replay_local(infx_stream* s, int32_t nshards, uint32_t nd, const infx_hit* all_hits /* nshards x nd x depth */, const uint32_t* all_hitcounts,
                                const float* all_next, int32_t depth, uint64_t* blob_bytes);
int32_t infx_shard_replay_blob(infx_stream* s, void* dst, uint64_t padded_bytes);
int32_t infx_shard_replay_merge(infx_stream* s, int32_t nshards, uint32_t nd, const void* all_blobs /* nshards x padded_bytes */, uint64_t padded_bytes, int32_t depth,
                                infx_hit* hits_out, uint32_t* hitcount_out);
int32_t infx_shard_replay_chain(infx_stream* s, uint32_t nd, const uint32_t* need, int32_t depth, void* state);
int32_t infx_shard_stage2(infx_stream* s, int32_t nshards, uint32_t nd, const infx_hit* all_hits /* nshards x nd x depth */, const uint32_t* all_hitcounts,
                          uint32_t nq, const infx_fused_query* fq, const infx_cov_query* cq, uint32_t nlists, const infx_wm_list* lists,
                          uint32_t owned_n, const int32_t* owned, int32_t depth, int32_t max_results, int32_t want_debug, infx_cov_out* outs_out);
int32_t infx_shard_finalize(infx_stream* s, uint32_t nq, const infx_cov_out* merged_outs, int32_t depth, int32_t max_results,
                            int64_t* out_keys, float* out_scores, uint8_t* out_ties, uint32_t* out_counts, uint32_t* out_flags);

/* After an infx_search_fused call with want_debug != 0: the intermediate device results (parity tests / introspection).
 * s1: nq x depth (ConsolidateSegments order) + counts; cands/outs/feat: nq x 2*depth rows, cand_counts[i] of them valid;
 * idx01: nq x 2 (documents with docIndex 0 / 1, -1 if absent).  Any pointer may be NULL. */
int32_t infx_fused_debug(infx_stream* s, infx_hit* s1, uint32_t* s1_counts, infx_cov_cand* cands, infx_cov_out* outs, int32_t* feat,
                         uint32_t* cand_counts, uint32_t* run_cov, int32_t* idx01);
/* kernel durations of the last fused call: accumulate, rules+select, prep2, stage2, finalize */
int32_t infx_last_fused_timings(infx_stream* s, float* ms5);
/* totals of the last fused call: Stage-1 rows kept, Stage-2 candidate rows scored, UTF-16 bytes of their texts */
int32_t infx_last_fused_stats(infx_stream* s, uint64_t* s1_rows, uint64_t* stage2_rows, uint64_t* stage2_text_bytes);

int32_t infx_last_timings(infx_stream* s, float* accumulate_ms, float* select_ms, float* stage2_ms);
/* Bytes the last accumulate launch actually streamed (posting slices of the doc ranges that held candidates: 5 B/posting,
 * 4 B for virtual terms, + 12 B per emitted arena entry) — an implementation figure, <= the algorithmic bytes of SURVEY 8(d). */
int32_t infx_last_alg_bytes(infx_stream* s, uint64_t* bytes);
/* Sum over the batch of card(C_q): candidates the tier rules let through (upper bound +128/query in disjunctive mode). */
int32_t infx_last_candidates(infx_stream* s, uint64_t* n);
/* Queries of the last batch whose Stage-1 cut was ambiguous and was replayed with the reference's sequential semantics (k_exact1). */
int32_t infx_last_exact_replays(infx_stream* s, uint32_t* n);
/* ... of them handed to the sequential k_exact1 by the parallel replay (k_mark_wide, k_ex_theta, k_ex_heap); 0 where the parallel replay does not run
 * (INFX_EXACT_SLOW=1, max_depth > 512: k_exact1 then takes every flagged query as it is). */
int32_t infx_last_exact_fallbacks(infx_stream* s, uint32_t* n);
/* The replay of the last batch: duration of its kernels (ms, HIP events on the stream) and why k_select flagged the queries:
 * why3[0] exact plateau (equal first-pass scores on both sides of the cut), [1] the best row left out lies inside the rounding band below the cut,
 * [2] the best row left out was not gathered (flagged conservatively). */
int32_t infx_last_replay_stats(infx_stream* s, float* ms, uint32_t* why3);
/* ... and its parts: the scan (k_ex_walk x2 + k_ex_prefix + k_ex_theta), k_ex_chunk (three launches), k_ex_heap, k_exact1 (ms, HIP events on the stream). */
int32_t infx_last_replay_breakdown(infx_stream* s, float* ms4);

#ifdef __cplusplus
}
#endif
#endif
