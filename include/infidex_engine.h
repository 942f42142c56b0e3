/*
 * infidex_engine.h — C ABI of the host engine inside libinfidex_hip.so.
 *
 * The reference's host is C# (src/Infidex/SearchEngine.cs); this image has no .NET toolchain, so the host side above the
 * device ABI (infidex_hip.h) is C++ and is exported here with the same surface for the hot path:
 *   SearchEngine.CreateDefault()/CreateMinimal()  SearchEngine.cs:78-94   -> infx_engine_create
 *   SearchEngine.IndexDocuments(IEnumerable<Document>)  :96-192           -> infx_engine_index_documents
 *   SearchEngine.Search(Query)                          :256-319          -> infx_engine_search_batch (one Query per row;
 *        Query.MaxNumberOfRecordsToReturn / CoverageDepth / EnableCoverage, Api/Query.cs:19,28,40)
 *   SearchEngine.Dispose                                 :477             -> infx_engine_destroy
 * A C# SearchEngine shim would call either this layer or infidex_hip.h directly.
 * All functions return int32 status (INFX_OK = 0) unless documented otherwise; infx_engine_last_error() gives the text.
 */
#ifndef INFIDEX_ENGINE_H
#define INFIDEX_ENGINE_H
#include "infidex_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct infx_engine infx_engine;

typedef struct infx_engine_config {
    int32_t device;           /* HIP device ordinal; -1 = host-only engine (indexing / planning introspection; Search fails) */
    int32_t range_docs;       /* see infx_config */
    int32_t max_depth;        /* largest Query.CoverageDepth (default 500) */
    int32_t threads;          /* host threads for indexing / query preparation; 0 = infx_engine_effective_cpus() */
    int32_t enable_coverage;  /* CreateDefault: 1, CreateMinimal: 0 */
    int32_t word_matcher;     /* CreateDefault: 1 (config 400 WordMatcherSetup), CreateMinimal: 0 */
    int32_t stop_term_limit;  /* 0 = 1 250 000 */
    int32_t want_features;    /* 1: Stage 2 also returns the integer feature vector (parity tests) */
    int32_t no_exact_replay;  /* 1: INFX_CFG_NO_EXACT_REPLAY (infidex_hip.h) — Stage-1 cut ties by (score, doc id) instead of the reference's heap order */
} infx_engine_config;

const char* infx_engine_last_error(void);
int32_t infx_engine_create(const infx_engine_config* cfg, infx_engine** out);
void    infx_engine_destroy(infx_engine* e);

/* n documents x field_count fields; field k of document d is arena[offs[d*field_count+k] .. offs[d*field_count+k+1]) (UTF-16);
 * field_weights[k] in {0 High, 1 Med, 2 Low} (Api/Weight.cs); keys == NULL means DocumentKey = document index. */
int32_t infx_engine_index_documents(infx_engine* e, int64_t n, const int64_t* keys, const uint16_t* arena, const uint64_t* offs,
                                    int32_t field_count, const int32_t* field_weights);

/* out_keys/out_scores/out_ties: nq x max_results (row-major); out_counts: nq; out_flags (may be NULL): bit0 query needs the
 * short-query path or exceeds the Stage-2 query envelope (empty result), bit1 coverage stage ran, bit2 coverage returned nothing -> Stage-1
 * fallback, bit3 a candidate document was left out of the ranking: the batch's over-long documents (> INFX_MAX_DOC_TOKENS words) exceeded the token-table pool. */
int32_t infx_engine_search_batch(infx_engine* e, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, int32_t max_results,
                                 int32_t depth, int32_t enable_coverage, int64_t* out_keys, float* out_scores, uint8_t* out_ties,
                                 uint32_t* out_counts, uint32_t* out_flags);

/* Sessions: one in-flight batch each (own HIP stream + scratch). Calling infx_engine_session_search_batch from several host
 * threads, one session per thread, overlaps the host preparation of one batch with the GPU stages of another — the
 * reference's concurrent-reader model (ReaderWriterLockSlim read lock, SearchEngine.cs:33,258). */
typedef struct infx_session infx_session;
int32_t infx_engine_session_create(infx_engine* e, infx_session** out);
void    infx_engine_session_destroy(infx_session* s);
int32_t infx_engine_session_search_batch(infx_session* s, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, int32_t max_results,
                                         int32_t depth, int32_t enable_coverage, int64_t* out_keys, float* out_scores, uint8_t* out_ties,
                                         uint32_t* out_counts, uint32_t* out_flags);
int32_t infx_engine_session_last_timings(infx_session* s, double* host_ms5, float* kernel_ms5, uint64_t* alg6);
/* exact Stage-1 replay of the session's last batch: kernel milliseconds (part of kernel_ms5[1]) and the k_select flag reasons (infx_last_replay_stats) */
/* Where the last batch's planning time went (ms): [0] text preparation + term lookups incl. the LD1 expansion call, [1] of that inside infx_ld1_expand
 * (device work and the wait for it), [2] inside infx_union_build (ditto), [3] idf / roles / device records. */
int32_t infx_engine_session_plan_breakdown(infx_session* S, double* out4);
int32_t infx_engine_session_replay_breakdown(infx_session* S, float* ms4 /* scan (k_ex_walk x2 + k_ex_prefix + k_ex_theta), k_ex_chunk, k_ex_heap, k_exact1 of the last batch */);
int32_t infx_engine_session_last_replay(infx_session* s, float* ms, uint32_t* why3);
/* HIP streams the session launches on, by priority (infx_stream_budget) */
int32_t infx_engine_session_stream_budget(infx_session* s, int32_t* normal, int32_t* high);
/* The main hipStream_t of a session / of the engine's own session (infx_engine_search_batch).  Main streams come from the device's pool of INFX_MAIN_STREAMS (default 4)
 * streams, fewest users first: the engine's own session is created first and takes the first, so with four sessions it shares that stream with the fourth.  Users of one
 * stream run in order on it: their batches serialise, and the per-phase kernel times of one (infx_engine_session_last_timings) include the other's kernels queued in
 * between.  That costs nothing while the engine's own session is idle, which is the intended use once sessions exist. */
int32_t infx_engine_session_stream_native(infx_session* s, void** hip_stream);
int32_t infx_engine_stream_native(infx_engine* e, void** hip_stream);

/* Document-sharded operation: every rank indexes the whole corpus on the host (global df / avgdl / N), uploads
 * its contiguous doc range, and a batch runs as four phases with the collectives in between:
 *   phase0 (text prep, LD1 member lists, k_union_count) -> all-reduce(sum) of infx_session_union_counts    [Exchange 1b: fuzzy df]
 *   phase1 (idf/roles + k_accumulate)  -> all-reduce(sum) of infx_session_counts (ndev x INFX_NCLASS)     [Exchange 1]
 *   phase2 (k_select, global counts) -> all-gather of hits (ndev x depth) and hit counts                  [Exchange 2, RCCL over xGMI]
 *   phase3 (merge to the global top-depth, Stage-2 prep, k_stage2 on the OWNED candidates)
 *          -> all-reduce(sum) of infx_session_outs (ncand x 3 int32; every candidate is scored by exactly one shard)
 *   phase4 (final ordering / truncation). */
/* SynonymMap.AddSynonym (Synonyms/SynonymMap.cs:33-62), before infx_engine_index_documents: index text, query text and coverage text are
 * canonicalised with the map (UTF-16 terms). */
int32_t infx_engine_add_synonym(infx_engine* e, const uint16_t* a, int32_t la, const uint16_t* b, int32_t lb);
int32_t infx_engine_set_shard(infx_engine* e, int32_t rank, int32_t nranks);      /* before infx_engine_index_documents */
int32_t infx_engine_shard_info(infx_engine* e, int32_t* doc_base, int32_t* num_docs);
int32_t infx_engine_default_session(infx_engine* e, infx_session** out);
int32_t infx_session_phase0(infx_session* s, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, int32_t depth, uint32_t* nunions);
int32_t infx_session_union_counts(infx_session* s, uint32_t* counts);
int32_t infx_session_phase1(infx_session* s, const uint32_t* global_union_counts, uint32_t* ndev);
int32_t infx_session_counts(infx_session* s, uint32_t* counts);
int32_t infx_session_phase2(infx_session* s, const uint32_t* global_counts, infx_hit* hits, uint32_t* hitcounts);
/* phase 2 in three steps for the exact cut across shards (infidex_hip.h, infx_shard_replay_*); every buffer may be host or device memory:
 *   phase2a: tier rules + first-pass top-`depth` + best score left out                 -> all-gather (hits, hitcounts, next)
 *   phase2b: global ambiguity test + this shard's part of the replay; *blob_bytes      -> max over ranks; infx_session_phase2b_blob -> all-gather
 *   phase2c: owner-side heap replay; hits / hitcounts = this rank's contribution         -> all-gather -> phase 3
 *   phase2d: (only if a hitcount is 0xFFFFFFFF) sequential chain step for the queries with need[q] != 0 */
int32_t infx_session_phase2a(infx_session* s, const void* global_counts, void* hits, void* hitcounts, void* next);
int32_t infx_session_phase2b(infx_session* s, int32_t nranks, const void* all_hits, const void* all_hitcounts, const void* all_next, uint64_t* blob_bytes);
int32_t infx_session_phase2b_blob(infx_session* s, void* dst, uint64_t padded_bytes);
int32_t infx_session_phase2c(infx_session* s, int32_t nranks, const void* all_blobs, uint64_t padded_bytes, void* hits, void* hitcounts);
int32_t infx_session_phase2d(infx_session* s, const uint32_t* need, void* state);
/* ---- native driver of the sharded phases -------------------------------------------------------------------------------------------------------------
 * Everything after phase 0 of a batch — phases 1, 2a-2d, 3, 4 with every collective in between — in ONE call, driven from C++ with no interpreter on the
 * path.  The collectives come through an infx_comm:
 *   infx_engine_comm_rccl : RCCL inside the library (infidex_hip.h: infx_set_shard_comm).  Exchange buffers live in HBM, the collectives are enqueued on the
 *                           session's HIP stream between the kernels that produce and consume them; the host synchronises only where it needs a value
 *                           (global fuzzy df for idf, the padded blob size, the "needs the sequential chain" flags).
 *   caller-supplied ops   : any other transport (the tests pass torch.distributed/gloo callbacks; device_buffers = 0: host exchange buffers).
 * Results are those of the phase-by-phase API (infidex_amd/sharded.py drives either). */
typedef struct infx_comm {
    void*   ctx;
    int32_t rank, nranks;
    int32_t device_buffers;      /* 1: buffers handed to the ops are device memory and the ops are stream-ordered on `stream`; 0: host memory, blocking ops */
    int32_t reserved;
    int32_t (*allreduce_sum_u32)(void* ctx, void* buf, uint64_t count, void* stream);                       /* in place */
    int32_t (*allgather)(void* ctx, const void* send, void* recv, uint64_t bytes_per_rank, void* stream);   /* recv: nranks x bytes_per_rank */
} infx_comm;
int32_t infx_engine_rccl_unique_id(void* id128);                                  /* rank 0: 128 bytes to ship to every rank */
int32_t infx_engine_comm_rccl(infx_engine* e, const void* id128, infx_comm* out);  /* every rank, after infx_engine_index_documents */
int32_t infx_session_comm_rccl(infx_session* s, const void* id128, infx_comm* out); /* a communicator per session: several batches in flight per rank */
/* phase 0 first (infx_session_phase0, possibly on a planner thread); then this call, in the same order on every rank */
int32_t infx_session_sharded_finish(infx_session* s, const infx_comm* comm, int32_t max_results, int32_t enable_coverage,
                                    int64_t* out_keys, float* out_scores, uint8_t* out_ties, uint32_t* out_counts, uint32_t* out_flags);

/* Collective order across a rank's pipeline sessions.  Each session has its own communicator and HIP stream; left alone, the order in which the sessions' host
 * threads enqueue their collectives — hence the relative order of different communicators' kernels on the device — depends on thread timing and differs between
 * ranks (the multi-communicator hang).  infx_engine_coll_ring declares the sessions of the coming stream (batch i on sessions[i mod n], the same on every rank):
 * inside infx_session_sharded_finish they then take turns, one collective per turn, in ring order; a session calls infx_session_coll_retire after its last batch
 * of the stream.  n = 0: no ordering.  INFX_COLL_ORDER=0 switches it off. */
int32_t infx_engine_coll_ring(infx_engine* e, uint32_t n, infx_session* const* sessions);
int32_t infx_session_coll_retire(infx_session* s);
int32_t infx_session_coll_stats(infx_session* s, uint64_t* out4 /* all-reduce calls, all-gather calls, all-reduce bytes, all-gather bytes; cumulative */);
int32_t infx_session_phase3(infx_session* s, int32_t nranks, const infx_hit* all_hits, const uint32_t* all_hitcounts, int32_t max_results,
                            int32_t enable_coverage, uint64_t* ncand);
int32_t infx_session_outs(infx_session* s, int32_t* outs3);
/* the same phases with caller-owned exchange buffers on the host OR the device (nd x depth hits + nd counts; nshards x ... ; nq x 2*depth
 * rows of 3 int32): with device tensors the collectives (RCCL) work in place and nothing crosses PCIe. infx_session_phase4 accepts either. */
int32_t infx_session_phase1x(infx_session* s, const uint32_t* global_union_counts, void* counts /* nq x INFX_NCLASS, host or device */, uint32_t* ndev);
int32_t infx_session_phase2x(infx_session* s, const uint32_t* global_counts /* host or device */, void* hits, void* hitcounts);
int32_t infx_session_phase3x(infx_session* s, int32_t nranks, const void* all_hits, const void* all_hitcounts, int32_t max_results, int32_t enable_coverage, void* outs);
int32_t infx_session_phase4(infx_session* s, const int32_t* merged_outs3, int64_t* out_keys, float* out_scores, uint8_t* out_ties,
                            uint32_t* out_counts, uint32_t* out_flags);

/* host_ms5: plan; Stage 1 incl. transfers (phase API only, 0 for the fused pipeline); Stage-2 preparation (fused pipeline:
 * WordMatcher list descriptors + PrepareQuery); GPU stage (phase API: Stage 2 incl. transfers; fused: the whole device
 * pipeline, one synchronisation); final ordering on the host (phase API only);
 * kernel_ms5: accumulate, rules + select, stage2, and for the fused pipeline candidate assembly (k_prep2) and final ordering
 * (k_finalize) — kernel durations from HIP events on the launch stream;
 * alg (6 entries): algorithmic bytes of the accumulate launch per SURVEY 8(d), Stage-2 candidate count, Stage-2 text bytes,
 * bytes the accumulate launch actually streamed, Stage-1 candidates, queries replayed by k_exact1. */
int32_t infx_engine_last_timings(infx_engine* e, double* host_ms5, float* kernel_ms5, uint64_t* alg6);

/* ---- introspection used by the parity tests (host logic runs without a GPU) ---- */
int32_t infx_engine_index_stats(infx_engine* e, int64_t* n_docs, int64_t* n_terms, int64_t* n_postings, float* avgdl);
int32_t infx_engine_export_index(infx_engine* e, int32_t* df, uint64_t* post_off, int32_t* post_doc, uint8_t* post_w, float* doc_len);
int32_t infx_engine_term_text(infx_engine* e, int32_t t, uint16_t* out, int32_t cap);
int32_t infx_engine_match_ld1(infx_engine* e, const uint16_t* q, int32_t len, int32_t* out, int32_t cap);
int32_t infx_engine_match_ld1_forward(infx_engine* e, const uint16_t* q, int32_t len, int32_t* out, int32_t cap);
int32_t infx_engine_plan(infx_engine* e, const uint16_t* q, int32_t len, int32_t depth, int32_t* term_ids, int32_t* dfs, float* idfs,
                         uint8_t* roles, uint8_t* ranks, int32_t cap, int32_t* meta5, int32_t* flags);
int64_t infx_engine_wordmatcher(infx_engine* e, const uint16_t* q, int32_t len, int32_t* out, int64_t cap);
/* The LD1 / WordMatcher lookups of planning as the DEVICE answers them (infidex_hip.h "Dictionary lookups"; uploaded by IndexDocuments unless
 * INFX_HOST_LOOKUPS=1).  _match_ld1_device: like _match_ld1 (count, first `cap` term ids in ordinal order); -1 / -2 = the kernel handed the word back to the
 * host (work lists outgrown / length outside 1..64).  _wordmatcher_device: like _wordmatcher (ascending unique doc ids over all of the query's lists). */
int32_t infx_engine_device_lookups(infx_engine* e);
int32_t infx_engine_lookup_stats(infx_engine* e, int64_t* out4 /* LD1 words on device / on host, WordMatcher queries on device / on host */);
int32_t infx_engine_match_ld1_device(infx_engine* e, const uint16_t* q, int32_t len, int32_t* out, int32_t cap);
int64_t infx_engine_wordmatcher_device(infx_engine* e, const uint16_t* q, int32_t len, int32_t* out, int64_t cap);
int32_t infx_engine_prefix_pop(infx_engine* e, const uint16_t* p, int32_t len);
int32_t infx_engine_last_stage1(infx_engine* e, uint32_t qi, int64_t* keys, float* scores, int32_t cap);
int64_t infx_engine_last_stage2(infx_engine* e, uint32_t* query_of, int32_t* docs, float* base, float* scores, uint8_t* ties,
                                int32_t* feat, int64_t cap);
/* CPUs usable by this process: hardware threads capped by the affinity mask and the cgroup CPU quota (INFX_THREADS overrides);
 * the default size of the host worker pool and of `threads`. */
/* ---- Document.Deleted ----------------------------------------------------------------------------------------------------------------------
 * DocumentCollection.DeleteDocumentsByKey (Core/DocumentCollection.cs:200-212): marks every document with one of the keys as deleted; the
 * index statistics are not rebuilt (as in the reference until the next re-index).  Searches skip deleted documents where the reference does
 * (Bm25Scorer.cs:322-323,455-459,622-624; SearchPipeline.cs:404-406,463-465,532-537).  Exclusive — no search in flight (the reference's write
 * lock).  On a sharded engine every rank must make the same call.  *out_marked (optional) = documents newly marked. */
int32_t infx_engine_delete_documents(infx_engine* e, const int64_t* keys, int64_t n, int64_t* out_marked);
/* SearchEngine.Load (SearchEngine.cs:399-441) of an INFDX2 file written by SearchEngine.Save (Indexing/IndexPersistence.cs:33-99): header and data
 * checksums are verified, the host index is built from the documents { DocumentKey, IndexedText as the single Med-weight field "content", Deleted }
 * and — BEFORE anything is uploaded — compared with what the file stores: every stored term (text, document frequency, postings with their weight
 * bytes; both ways) and every derived section the reference's Load would read and search with (csrc/host/infdx2_verify.h): the term FST (every term
 * with its collection index, forward and reverse trie in FstBuilder's layout), the short-query index (every (prefix, document, token position) entry
 * regenerated from the index texts), the document metadata cache (first token, token count) and the WordMatcher section behind the checksum (exact and
 * symmetric-delete dictionaries with their Roaring document sets, the affix FST with its last-occurrence documents).  A WordMatcher section on an engine
 * configured without one, or none on an engine configured with one, is refused as SearchEngine.cs:436-439 throws.
 * checked3 (optional): documents, stored terms compared, stored postings compared.  INFX_EUNSUPPORTED when a stored structure is not what the builder
 * produces for the stored texts (e.g. written from differently weighted fields, another stop-term limit, a derived section that says something else than
 * the documents) — the engine is left unindexed and can load another file; INFX_EINVAL for a foreign or corrupted file. */
int32_t infx_engine_load_index(infx_engine* e, const char* path, int64_t* checked3);
/* SearchEngine.Flush's on-disk segments (INFS: Indexing/Segments/SegmentWriter.cs:13-94, BlockPostingsWriter.cs:24-161 — blocks of 64..256 delta-coded postings
 * with min / max doc and max weight per block, Compression/GroupVarInt.cs, the "FST2" term tries, Elias-Fano list offsets).  infx_segment_open reads and
 * VALIDATES a file (every offset, the skip tables against the decoded blocks, the tries against each other, the Elias-Fano select index); infx_segment_export hands its
 * content over as CSR in ordinal term order — term texts (UTF-16 arena + offsets) and, per term, ascending segment-local doc ids with their weight bytes: the layout
 * infx_upload_postings takes (map the ordinals to the host's term ids first).  Any output pointer may be NULL. */
typedef struct infx_segment infx_segment;
int32_t infx_segment_open(const char* path, infx_segment** out);
void    infx_segment_close(infx_segment* seg);
int32_t infx_segment_info(infx_segment* seg, int32_t* doc_count, int32_t* num_terms, int64_t* num_postings, int64_t* term_chars);
int32_t infx_segment_export(infx_segment* seg, uint32_t* term_offs /* T+1 */, uint16_t* term_chars, uint64_t* post_offs /* T+1 */, int32_t* doc_ids, uint8_t* weights);
/* A flushed segment against the engine's index of the same documents: the segment covers the documents [doc_base, doc_base + its docCount) (VectorModel.Flush writes
 * ids relative to the documents flushed before, VectorModel.cs:804-815).  Every term of the segment must exist in the index with exactly the segment's (document,
 * weight) postings inside that range, and every index term with postings in the range must be in the segment.  checked3 (optional): documents, terms, postings
 * compared.  INFX_EINVAL for a foreign or corrupted file, INFX_EUNSUPPORTED when segment and index disagree. */
int32_t infx_engine_verify_segment(infx_engine* e, const char* path, int32_t doc_base, int64_t* checked3);
/* An engine populated from FLUSHED SEGMENTS + a live tail instead of infx_engine_index_documents (VectorModel.Flush, Indexing/VectorModel.cs:804-815;
 * Indexing/Segments/SegmentReader.cs): segment i holds the postings of documents [doc_bases[i], doc_bases[i] + its document count); the segments cover the
 * documents from 0 without gaps, in order; documents behind the last segment are the live tail.  All n documents are supplied and accumulated (term ids, the
 * df counter with its double counts on saturated weight bytes, the stop-term decisions, document lengths, WordMatcher dictionaries and Stage-2 texts need them: a
 * segment stores none of that); the segments' (document, weight) postings then replace the accumulated ones of their ranges, list by list, and must name exactly
 * the documents the accumulation found (a term without a list in a segment was a stop term at flush time and stays one).
 * The corpus is then searched as ONE index (= an unflushed index of the same documents), not segment by segment as VectorModel.cs:572-584 does.
 * INFX_EUNSUPPORTED: a segment written from other documents; the engine stays unindexed. */
int32_t infx_engine_index_from_segments(infx_engine* e, int64_t n, const int64_t* keys, const uint16_t* arena, const uint64_t* offs, int32_t field_count, const int32_t* field_weights,
                                        int32_t n_segments, const char* const* paths, const int32_t* doc_bases);
int32_t infx_engine_restore_documents(infx_engine* e);      /* clears every Deleted flag */
/* Document.Deleted = true on single documents by internal id (indexing order), e.g. one of several documents of a key; otherwise as
 * infx_engine_delete_documents.  The documents of one key then differ in their flag, which deletion by key never produces: browse rows and the
 * whole-corpus facets are held to the reference in that state (first live document of the key); the text-query paths skip each Deleted document as
 * they always do, but their key lookups (consolidation, post-filter, facets) have no test on a key that is partly deleted. */
int32_t infx_engine_delete_document_ids(infx_engine* e, const int64_t* ids, int64_t n, int64_t* out_marked);
/* One host-index build per node instead of one per rank (document shards: every process needs the whole host index — global df / avgdl / N, the term and
 * word dictionaries, the WordMatcher lists).  The node's leader indexes the documents (infx_engine_set_build_threads lets that build use every
 * core of the node while planning keeps the rank's share), saves the host index to a node-local file (e.g. under /dev/shm) and the other ranks call
 * infx_engine_index_from_host_cache INSTEAD of infx_engine_index_documents: they read the arrays back and upload their own shard.  The file pins its
 * layout version, the configuration (n-gram, stop-term, WordMatcher, synonym settings), the index fingerprint and a checksum of its payload; anything
 * else is refused (INFX_EINVAL).  It is created exclusively (O_EXCL | O_NOFOLLOW, mode 0600) and read without following a link.  A transient hand-off between the processes of one build — not the reference's INFDX2 format (infx_engine_load_index). */
int32_t infx_engine_set_build_threads(infx_engine* e, int32_t threads);     /* 0 = the engine's thread count */
int32_t infx_engine_save_host_index(infx_engine* e, const char* path);
int32_t infx_engine_index_from_host_cache(infx_engine* e, const char* path);

/* ---- Query.Filter (Infiscript, Api/FilterParser.cs) and Query.EnableFacets (config 5) -------------------------------------------------
 * Non-indexed document fields are given as columns (one value per indexed document, in indexing order); the post-filter of the returned
 * rows (Scoring/ResultProcessor.cs:35-70), Filter.NumberOfDocumentsInFilter and the facet counts (Core/FacetBuilder.cs:19-105) run on the
 * device (include/infidex_hip.h).  kind: 1 int64, 2 double, 3 UTF-8 strings (arena + n+1 offsets).  A name the engine already holds REPLACES
 * that column in its slot (new values, possibly of another kind): compiled filters, filter counts, masks, filtered-facet answers and the column's
 * sort rank are built again on their next use.  An exclusive call, like indexing: no search is in flight.  The name must not be empty (INFX_EINVAL): a
 * nameless slot is what a scalar column leaves behind when a list column takes its name (below). */
int32_t infx_engine_add_column(infx_engine* e, const char* name, int32_t kind, int32_t facetable, int64_t n, const int64_t* vals_i, const double* vals_d,
                               const char* arena, const uint64_t* offs);
int32_t infx_engine_column_count(infx_engine* e);
int32_t infx_engine_column_info(infx_engine* e, int32_t col, char* name, int32_t cap, int32_t* facetable, int32_t* num_values);
int32_t infx_engine_column_value(infx_engine* e, int32_t col, uint32_t code, char* out, int32_t cap);
/* ---- list columns: a field that holds a LIST of values per document (Field.IsArray: genres, tags, authors) ---------------------------------------------
 * infx_engine_add_list_column gives one list per indexed document, in indexing order: doc_offs[n + 1] (ascending from 0) delimits document d's elements,
 * which are vals_i (kind 1), vals_d (kind 2) or the strings arena[offs[j] .. offs[j + 1]) (kind 3) — kinds as in infx_engine_add_column; all elements of a
 * column are of one kind.  Lists are kept as given: order and duplicates stay.  The elements are dictionary-encoded like a scalar column's values; the device
 * holds the lists as a CSR pair of uint32 (fewer than 2^32 elements per column: INFX_ECAPACITY beyond).
 * Names: list columns and scalar columns share ONE namespace — a name that either kind holds is replaced by the new column, of either kind, with the
 * invalidation documented for infx_engine_add_column (a scalar column replaced by a list column leaves its slot behind as a nameless column that the next
 * new scalar column takes).  List columns take no slot among the 64 scalar columns and none among the INFX_MAX_FACET_COLS facet columns: there are at most
 * INFX_ENGINE_MAX_LIST_COLS of them, of which INFX_ENGINE_MAX_LIST_FACETS may be facetable (INFX_ECAPACITY beyond).  INFX_EUNSUPPORTED on a sharded engine.
 * FILTERS.  A leaf of the filter language over a list column holds for a document iff its list is not empty and the leaf holds for AT LEAST ONE element
 * (as it would for a scalar value), or its list is empty and the leaf holds for a null value: `tags IS NULL` accepts the empty lists (so do < and <=, for which a null is below every constant, as for a scalar field) and no other comparison does.
 * NOT, AND, OR and ?: apply to that verdict: `NOT tags = 'sale'` and `tags != 'sale'` (which is NOT over an = leaf) both mean "no element equals sale".
 * Such a leaf is lowered, on the first use of its expression, to a derived one-bit column on the device (k_list_leaf; all missing leaves of an expression
 * over one list column in one launch) that takes a free slot among the 64 scalar slots and is read by every kernel that runs filter programs like any
 * scalar column: post-filters, boosts, pre-filters, filtered facets, browse queries, listings and every aggregate's filter.  The engine caches at most
 * INFX_ENGINE_MAX_DERIVED derived columns by (list column, operator, constants), least recently used first out among those no cached compiled filter uses;
 * an expression that finds no entry or no slot free is refused alone with INFX_ECAPACITY.  infx_engine_last_list_leaf_stats: derived columns built and
 * k_list_leaf launches of the last expression the engine COMPILED (an expression taken from the filter cache compiles nothing and leaves them as they are);
 * infx_engine_list_leaf_totals: the same two figures summed over every compile of the engine — unchanged by a call that compiled or built nothing.
 * FACETS.  A facetable list column is counted by infx_engine_facets_all and infx_engine_facets_filtered (k_list_facets): a value's count is the number of its
 * element occurrences — a duplicate counts twice, as FacetBuilder counts it — among the live documents (the expression accepts); empty strings are left
 * out; order and cut as the scalar facets.  Readers: infx_engine_facets_all_list_column / infx_engine_facets_filtered_list_column, as their scalar
 * counterparts, with the list column's index in *lcol; names and values from infx_engine_list_column_info / _value.  totals count documents, not elements.
 * NOT BUILT: the facets of the returned rows (infx_engine_last_facets) and of a browse query do not include list columns; a list column named as order_by,
 * sort_by, group_by, collapse_by, field or bucket_by is refused for that request (query) alone, as an unknown field is; a session-wide
 * infx_engine_set_sort by a list column returns INFX_EINVAL.
 * infx_engine_list_column_document: the stored list of one document as element codes (up to cap; returns the list's length, -1 on error). */
#define INFX_ENGINE_MAX_LIST_COLS 8
#define INFX_ENGINE_MAX_LIST_FACETS 4
#define INFX_ENGINE_MAX_DERIVED 16
int32_t infx_engine_add_list_column(infx_engine* e, const char* name, int32_t kind, int32_t facetable, int64_t n, const uint64_t* doc_offs /* n+1 */,
                                    const int64_t* vals_i, const double* vals_d, const char* arena, const uint64_t* offs);
int32_t infx_engine_list_column_count(infx_engine* e);
int32_t infx_engine_list_column_info(infx_engine* e, int32_t lcol, char* name, int32_t cap, int32_t* facetable, int32_t* num_values, int32_t* kind);
int32_t infx_engine_list_column_value(infx_engine* e, int32_t lcol, uint32_t code, char* out, int32_t cap);
int64_t infx_engine_list_column_document(infx_engine* e, int32_t lcol, int64_t document_index, uint32_t* codes, int64_t cap);
int32_t infx_engine_last_list_leaf_stats(infx_engine* e, uint32_t* built, uint32_t* launches);
int32_t infx_engine_list_leaf_totals(infx_engine* e, uint64_t* built, uint64_t* launches);
int32_t infx_engine_facets_all_list_column_count(infx_session* s);
int32_t infx_engine_facets_all_list_column(infx_session* s, uint32_t k, int32_t* lcol, uint32_t* codes, uint32_t* counts, int32_t cap);
int32_t infx_engine_facets_filtered_list_column_count(infx_session* s);
int32_t infx_engine_facets_filtered_list_column(infx_session* s, uint32_t which, uint32_t k, int32_t* lcol, uint32_t* codes, uint32_t* counts, int32_t cap);
/* Post rows: how many returned rows per query the filter, facets, boosts, sort-by and browse rows accept — INFX_FILTER_MAX_ROWS (64, the default) up to
 * INFX_POST_MAX_ROWS (1024 = the largest max_depth, so no text query returns more).  The reference post-filters the truncated top-MaxNumberOfRecordsToReturn
 * rows (SearchEngine.cs:304-310): a caller who wants twenty rows that pass a selective filter asks for a few hundred.  An engine left at the default
 * behaves exactly as before, refusals at 65 rows included; queries of at most 64 rows run on the same one-wave kernels whatever the setting, wider ones
 * on workgroup-per-query kernels launched only for a batch that has one.  Legal between create and the first search (the sessions size their facet
 * readout by it); afterwards, and outside the range, INFX_EINVAL with a message. */
int32_t infx_engine_set_post_rows(infx_engine* e, int32_t rows);
int32_t infx_engine_get_post_rows(infx_engine* e, int32_t* out);
int32_t infx_engine_set_filter(infx_session* s, const char* expr_utf8 /* NULL = no filter */, int32_t enable_facets, uint32_t* n_in_filter);
int32_t infx_engine_facet_column_count(infx_session* s);
int32_t infx_engine_last_facets(infx_session* s, uint32_t nq, uint32_t qi, uint32_t k, int32_t* col, uint32_t* codes, uint32_t* counts, int32_t cap);
/* A query whose text is empty (or all whitespace) and that has EnableFacets — through infx_engine_set_filter(.., enable_facets = 1, ..) or its
 * infx_query_options — is a browse query (SearchEngine.HandleEmptyQueryWithFacets, SearchEngine.cs:321-346): it returns the first max_results documents
 * in indexing order that are not Deleted and whose key's first live document passes the filter, each with score 65535 and tiebreaker 0, and the facets
 * of those rows; Boosts, SortBy and coverage do not apply.  NumberOfDocumentsInFilter, the row limit (the engine's post rows, 64 by default) and the refusals are those of a text query.
 * Without EnableFacets (or without a facetable column) a blank query returns nothing, as before.
 *
 * FacetBuilder.BuildFacetsFromAllDocuments (Core/FacetBuilder.cs:110-181): infx_engine_facets_all counts, in one device pass, the values of every
 * facetable column (the first INFX_MAX_FACET_COLS) over all documents that are not Deleted — per document, not per key; *ncols = those columns.
 * infx_engine_facets_all_column then gives the k-th column's (code, count) pairs, count descending then value ascending, at most 100, null and empty
 * values left out; it returns their number, -1 on error.  INFX_EHIP on an engine without a GPU.
 * infx_engine_last_browse_stats: the groups (distinct filter programs, the counted ones included) and the k_browse_scan launches (256 groups each) of the
 * session's last batch that had a browse query. */
int32_t infx_engine_last_browse_stats(infx_session* s, uint32_t* groups, uint32_t* launches);
int32_t infx_engine_facets_all(infx_session* s, int32_t* ncols);
int32_t infx_engine_facets_all_column(infx_session* s, uint32_t k, int32_t* col, uint32_t* codes, uint32_t* counts, int32_t cap);
/* Query.EnableBoost + Query.Boosts (ResultProcessor.ApplyBoosts, Scoring/ResultProcessor.cs:75-121) for the following searches on the session: n boosts,
 * exprs[i] its Infiscript filter (NULL: a Boost whose Filter is null, dropped), strengths[i] = (int)BoostStrength (Low 1, Med 2, High 3).  enable = 0
 * (or n = 0) clears and compiles nothing.  Filters are compiled through the engine's filter cache; a boost never counts NumberOfDocumentsInFilter.
 * Status: INFX_EINVAL + message for a syntax error, INFX_EUNSUPPORTED for MATCHES, INFX_ECAPACITY for more than INFX_MAX_BOOSTS with a filter. */
int32_t infx_engine_set_boosts(infx_session* s, uint32_t n, const char* const* exprs, const int32_t* strengths, int32_t enable);
/* Query.SortBy / Query.SortAscending (ResultProcessor.ApplySort, :126-141): field = a column name (case sensitive; unknown: every row null), NULL = sort
 * by relevance.  The first use of a column builds its dense sort rank (CompareValues: int64 / double — NaN lowest, -0 == +0 — numerically, strings
 * OrdinalIgnoreCase then ordinal, PARITY UNPINNED) and uploads it to the device. */
int32_t infx_engine_set_sort(infx_session* s, const char* field, int32_t ascending);
/* ---- per-query options: SearchEngine.Search(Query) (SearchEngine.cs:256-362) for a batch of Query objects, each with its own options ----------------
 * infx_engine_set_query_options installs the options of the session's NEXT search of nq queries, whichever path runs it (infx_engine_session_search_batch,
 * INFX_PHASED, the sharded phases or infx_session_sharded_finish); that search consumes them.  The host phases (INFX_PHASED) have no device finalize:
 * there max_results and enable_coverage apply, and a query with a filter, facets, boosts or sort is refused on its own (INFX_EUNSUPPORTED, see below).  The search call's max_results is the row stride and must be
 * >= every query's (else INFX_EINVAL); its enable_coverage is ANDed with each query's; CoverageDepth stays one per call.  A query with no filter, facets,
 * boosts or sort behaves as in a plain batch.  A query is rejected on its own — empty result, result flag bit 4 (INFX_RESULT_REJECTED), its status in
 * out_status[i] and its message from infx_engine_query_error — for a filter syntax error (INFX_EINVAL), MATCHES (INFX_EUNSUPPORTED), more than
 * INFX_MAX_BOOSTS boosts with a filter (INFX_ECAPACITY), or post-processing on more rows than the engine's post rows (INFX_FILTER_MAX_ROWS unless infx_engine_set_post_rows raised them; INFX_EUNSUPPORTED; facets count as
 * post-processing only when a facetable column exists); its neighbours are unaffected.  Installing while a session-wide filter, facets, boosts or sort is installed (infx_engine_set_filter / _set_boosts / _set_sort) is
 * INFX_EINVAL, and so is the reverse; a search of another nq fails with INFX_EINVAL and clears the options.  nq = 0 clears.
 * Filter.NumberOfDocumentsInFilter: the expressions the batch uses for the first time are counted in one k_filter_count_multi launch enqueued with the
 * batch (no extra host wait); infx_engine_last_in_filter returns each query's count after the batch.  It counts every document of the WHOLE corpus that
 * is not Deleted, on every rank of a sharded engine (each holds the whole columns and the global Deleted flags): no collective, unlike
 * infx_engine_set_filter, which reports the shard's share.  Counts are cached per expression in the engine's filter cache (shared with
 * infx_engine_set_filter), its host entries bounded, least recently used first (infx_engine_set_filter_cache_limit, default 4096: the device copies that
 * infx_engine_set_filter / _set_boosts made of evicted entries are kept until the engine is destroyed); an installed entry is never evicted, an
 * evicted one is counted again on its next use.  Deletions and new columns invalidate the counts. */
typedef struct infx_query_options {
    int32_t max_results;                    /* MaxNumberOfRecordsToReturn */
    int32_t enable_coverage, enable_facets, enable_boost;
    const char* filter;                     /* Infiscript, UTF-8; NULL = none */
    uint32_t nboosts; const char* const* boost_filters; const int32_t* boost_strengths;      /* Boosts (a NULL filter: a Boost whose Filter is null, dropped) */
    const char* sort_by; int32_t sort_ascending;                                             /* SortBy (column name, NULL = relevance) / SortAscending */
} infx_query_options;
int32_t infx_engine_set_query_options(infx_session* s, uint32_t nq, const infx_query_options* opts, int32_t* out_status /* nq */);
/* NumberOfDocumentsInFilter of each query of the session's last per-query batch (0 for a query without a filter or rejected) */
int32_t infx_engine_last_in_filter(infx_session* s, uint32_t nq, uint32_t* out);
/* how many expressions the session's last per-query batch counted, and in how many kernel launches */
int32_t infx_engine_last_count_stats(infx_session* s, uint32_t* counted, uint32_t* launches);
/* why query qi of the session's coming batch, or of the batch just searched, is rejected: the message of the first part that refuses it among the ones installed
 * for that batch, in the order infx_engine_set_query_options, _set_query_coverage, _set_query_prefilters, _set_query_collapse, whichever was installed last ("" if
 * none refuses it); rewritten by each of the four calls and by the search that consumes them.  Returns its length, -1 out of range */
int32_t infx_engine_query_error(infx_session* s, uint32_t qi, char* out, int32_t cap);
/* ---- CoverageSetup (Coverage/CoverageSetup.cs): the Stage-2 settings, engine-wide and per query ---------------------------------------------------
 * infx_coverage_setup carries the 17 settable members (CoverageDepth is never read by the reference: Query.CoverageDepth is used instead).
 * ENGINE-WIDE (SearchEngine's coverageSetup: argument, SearchEngine.cs:51,64-67,74) — infx_engine_set_coverage_setup; NULL = CoverageSetup's defaults.  It feeds
 *   - the matchers (CoverageEngine._setup): min_word_size, the five cover_* switches, num_typos (above 2 behaves as 2), min_length_one_typo,
 *     min_length_two_typos, levenshtein_max_word_size;
 *   - the WordMatcher lookup: cover_prefix_suffix off = no affix matches (WordMatcherLookup.cs:51);
 *   - the defaults of the pipeline-level members below.
 *   Nothing built at index time depends on it, so the call is legal before or after infx_engine_index_documents and between batches (not while a search is
 *   in flight; on a sharded engine every rank makes the same call; plans prefetched for a coming batch keep the tokens they were made with).
 * PER QUERY (Query.CoverageSetup, `q.CoverageSetup ?? _coverageSetup`, SearchEngine.cs:300) — infx_engine_set_query_coverage installs the setups of the session's
 *   NEXT search of nq queries (setups[i] == NULL: the engine-wide setup), consumed by that search like infx_engine_set_query_options and usable with or without
 *   it, on every path it supports.  As in the reference a per-query setup replaces only what SearchPipeline itself reads — truncate, coverage_min_word_hits_abs,
 *   coverage_min_word_hits_relative, truncation_score, coverage_q_limit_for_error_tolerance, coverage_lcs_error_tolerance_relativeq; its matcher members are
 *   IGNORED: the matchers and the WordMatcher lookup keep the engine's object (quirk Q19).
 * Validation: integers outside [0, 65535], truncation_score outside [0, 255], a non-finite or negative relativeq -> INFX_EINVAL (per query: that query is
 * rejected on its own, see below).  enable_lexical_prescreen (LexicalPrescreen.cs) is not implemented: engine-wide it is refused with INFX_EUNSUPPORTED; a query
 * with it is rejected on its own like a MATCHES filter — empty result, result flag bit 4, its status in out_status[i], its message from infx_engine_query_error,
 * neighbours unaffected.  With coverage off (CreateMinimal engine, EnableCoverage = false) a setup has no effect. */
typedef struct infx_coverage_setup {
    int32_t min_word_size, levenshtein_max_word_size, num_typos, min_length_one_typo, min_length_two_typos;        /* 2, 20, 2, 3, 7 */
    int32_t coverage_min_word_hits_abs, coverage_min_word_hits_relative, coverage_q_limit_for_error_tolerance;       /* 1, 0, 5 */
    double  coverage_lcs_error_tolerance_relativeq;                                                                   /* 0.2 */
    int32_t cover_whole_query, cover_whole_words, cover_fuzzy_words, cover_joined_words, cover_prefix_suffix;        /* 1 each */
    int32_t truncate, enable_lexical_prescreen, truncation_score;                                                    /* 1, 0, 254 */
} infx_coverage_setup;
int32_t infx_coverage_setup_default(infx_coverage_setup* out);
int32_t infx_sizeof_coverage_setup(void);
int32_t infx_engine_set_coverage_setup(infx_engine* e, const infx_coverage_setup* setup /* NULL = defaults */);
int32_t infx_engine_get_coverage_setup(infx_engine* e, infx_coverage_setup* out);
int32_t infx_engine_set_query_coverage(infx_session* s, uint32_t nq, const infx_coverage_setup* const* setups, int32_t* out_status /* nq, may be NULL */);
/* ---- Query.pre_filter: rank only the documents a filter accepts -----------------------------------------------------------------------------------
 * Query.Filter is a post-filter (SearchEngine.cs:304-310): it runs on the truncated top rows.  A PRE-filter restricts the set that is ranked: a query with
 * pre-filter P returns what the same query returns on the same index if every document P does not accept carried Document.Deleted = true.  "Accept" is the
 * filter VM's three-valued evaluation of the document's own column values (only True accepts, an absent column is null) — what NumberOfDocumentsInFilter counts.
 * Index statistics (df, avgdl, N, stop terms) are untouched, as with deletions; real deletions stay in force; the mask is per document, not per key.  Filter,
 * EnableFacets, Boosts and SortBy then post-process the returned rows as without it.  A query without a pre-filter, alone or beside pre-filtered ones, runs
 * the code and returns the bits it would in a batch without any.
 * infx_engine_set_query_prefilters installs the pre-filters (Infiscript, UTF-8; exprs[i] == NULL: none) of the session's NEXT search of nq queries: consumed
 * by that search like infx_engine_set_query_coverage, usable with or without infx_engine_set_query_options, nq = 0 clears, a search of another nq fails with
 * INFX_EINVAL and clears them.  Expressions go through the engine's filter cache.  A query is rejected on its own — empty result, result flag bit 4, its
 * status in out_status[i], its message from infx_engine_query_error when its options were accepted, neighbours unaffected — for a syntax error (INFX_EINVAL),
 * MATCHES (INFX_EUNSUPPORTED), a 17th distinct pre-filter in one batch (INFX_ECAPACITY: split the batch), an empty text with EnableFacets (a browse query,
 * whose Filter already restricts the scan; known when the batch runs: the status then shows in the result flag and the message only), the host phases
 * (INFX_PHASED) and a sharded engine (INFX_EUNSUPPORTED each).
 * Masks: one byte per document, at most INFX_MAX_PREFILTERS (16) per session, keyed by the expression, least recently used first out, reused across batches.
 * The masks a batch is missing are built by ONE k_filter_mask_multi launch on the session's stream in front of the batch — no extra host wait, nothing shared
 * between sessions.  infx_engine_delete_documents / _delete_document_ids / _restore_documents / _add_column and indexing start a new mask epoch: every
 * session builds its masks again on next use. */
int32_t infx_engine_set_query_prefilters(infx_session* s, uint32_t nq, const char* const* exprs, int32_t* out_status /* nq, may be NULL */);
/* live documents each query's pre-filter accepts, of the session's last search (0 for a query without one, or rejected) */
int32_t infx_engine_last_in_prefilter(infx_session* s, uint32_t nq, uint32_t* out);
/* masks the session's last search (or infx_engine_prefilter_mask) built and took from its cache, and the k_filter_mask_multi launches that took */
int32_t infx_engine_last_prefilter_stats(infx_session* s, uint32_t* built, uint32_t* reused, uint32_t* launches);
/* Parity tooling: the mask of one expression as the device holds it — built, or taken from the session's cache — one byte per indexed document in
 * out_bytes (cap >= the number of documents): 1 = Deleted or not accepted. */
int32_t infx_engine_prefilter_mask(infx_session* s, const char* expr, uint8_t* out_bytes, uint64_t cap);
/* ---- Query.collapse_by: the best N ranked rows of every group (not in the reference; DESIGN.md "collapse_by") ----------------------------------------
 * What Elasticsearch calls collapse, Solr field collapsing and Algolia distinct: "at most one hit per product family", "no more than three results per shop".
 * For a query Q with collapse field F and keep N, let Q0 be Q without collapsing, Filter, EnableFacets, Boosts and SortBy and with MaxNumberOfRecordsToReturn =
 * CoverageDepth, and L the rows Q0 returns: the whole ranked list the pipeline has for the query (at most CoverageDepth <= 1024 rows, consolidated per key, cut
 * at the truncation index, the Stage-1 fallback rows where coverage returned nothing; with a pre-filter, of the documents it accepts).  A row's group is the
 * dictionary code, in column F, of the document whose score it carries — one code one group, as in infx_engine_list_groups; any column will do.  A row is kept
 * when fewer than N earlier rows of L have its group; kept rows stay in L's order with their scores and tiebreakers.  Q returns the first
 * MaxNumberOfRecordsToReturn kept rows with Q0's result flags; Filter, facets, Boosts and SortBy then work on those rows as they do on any query's, and the
 * post-rows limit is held against MaxNumberOfRecordsToReturn, not against L.  Truncation is decided on L, before anything is collapsed.
 * infx_engine_set_query_collapse installs fields[i] (a column name, UTF-8; NULL: query i is not collapsed; fields == NULL: none is) and keeps[i] (1 ..
 * INFX_COLLAPSE_MAX_KEEP) for the session's NEXT search of nq queries: consumed by that search like infx_engine_set_query_prefilters, usable with or without
 * infx_engine_set_query_options, nq = 0 clears, a search of another nq fails with INFX_EINVAL and clears them.  The caller's row stride and output arrays do not
 * grow: L lives in scratch of the session.  A query is rejected on its own — empty result, result flag bit 4, its status in out_status[i], its message from
 * infx_engine_query_error, neighbours unaffected — for an unknown column or a keep outside 1 .. 16 (INFX_EINVAL), an empty text with EnableFacets (a browse
 * query ranks nothing; known when the batch runs: the status then shows in the result flag and the message only), the host phases (INFX_PHASED) and a sharded
 * engine (INFX_EUNSUPPORTED each), an engine without a GPU (INFX_EHIP).  An empty text without facets stays an empty result without error.
 * A batch without a collapsing query launches the kernels it launched before with the arguments it passed before.
 *   infx_engine_last_collapse        per query of the session's last search (nq: its size) the distinct groups of L and the rows of L; 0 where none was folded
 *   infx_engine_collapse_rows        query qi's rows as returned (after Filter and SortBy): *col the collapse column, per row its group's code in that column
 *                                    (infx_engine_column_value gives the text) and the rows of L in its group, itself included; returns the rows written (at most
 *                                    cap), -1 on error or for a query that was not collapsed
 *   infx_engine_last_collapse_stats  collapsing queries and k_collapse launches of the session's last search: (k, 1) with k collapsing queries, (0, 0) without */
#define INFX_COLLAPSE_MAX_KEEP 16
int32_t infx_engine_set_query_collapse(infx_session* s, uint32_t nq, const char* const* fields /* NULL: none */, const int32_t* keeps, int32_t* out_status /* nq, may be NULL */);
int32_t infx_engine_last_collapse(infx_session* s, uint32_t nq, uint32_t* total_groups, uint32_t* total_ranked);
int32_t infx_engine_collapse_rows(infx_session* s, uint32_t qi, int32_t* col, uint32_t* codes, uint32_t* sizes, int32_t cap); /* rows written, -1 on error */
int32_t infx_engine_last_collapse_stats(infx_session* s, uint32_t* queries, uint32_t* launches);
/* ms2[0] k_finalize's and ms2[1] k_collapse's duration in the session's last search (HIP events on its stream; zeros when nothing was collapsed) */
int32_t infx_engine_last_collapse_timings(infx_session* s, float* ms2);
/* ---- Query.highlight: match spans and a snippet for every returned row (not in the reference; DESIGN.md "highlight") ---------------------------------
 * What Elasticsearch calls highlight and Algolia _highlightResult: per returned row, which document word each query word matched and how, every occurrence
 * of those words (the spans a UI paints) and a snippet of the stored text around them.  The match is Stage 2's: its four matchers (whole word, joined words,
 * prefix / suffix / infix / tail, fuzzy prefix and fuzzy) over the stored text lower(normalize(IndexedText)) — infx_engine_document_text —, with the engine's
 * CoverageSetup, alias folding and dedupe; a pure function of the query's Stage-2 words, that text and those settings, whatever the row's score came from
 * (Stage-1 fallback rows and queries without coverage are highlighted too).  Offsets and lengths are UTF-16 units of the stored text, not of the input.
 * infx_engine_set_query_highlight installs chars[i] (0: query i does not ask; else its snippet width, INFX_HIGHLIGHT_MIN_CHARS .. INFX_HIGHLIGHT_MAX_CHARS) for
 * the session's NEXT search of nq queries: the fifth part of the per-query frame, behind the collapse requests — consumed by that search, usable with or without
 * infx_engine_set_query_options, nq = 0 (or chars == NULL) clears, a search of another nq fails with INFX_EINVAL and clears it.  A query is rejected on its own
 * (empty result, result flag bit 4, its status in out_status[i], its message from infx_engine_query_error, neighbours unaffected) for a width out of range
 * (INFX_EINVAL), an empty text with EnableFacets (a browse query matched nothing; known when the batch runs), the host phases (INFX_PHASED) and a sharded
 * engine (INFX_EUNSUPPORTED each), an engine without a GPU (INFX_EHIP).  A batch without a highlighting query launches and downloads what it did before.
 * Limits of this version, stated per row and never silent: a document of more than INFX_MAX_DOC_TOKENS (192) Stage-2 words has status 1 ("too_long"), a query
 * outside the fast envelope (more than INFX_MAX_QUERY_TOKENS words or INFX_MAX_QUERY_CHARS characters) status 2 ("long_query") on every row.
 *   infx_engine_highlight_query        of highlighted query qi of the session's last search: its rows, the batch's term and snippet strides, whether it is a
 *                                      long query, and its Stage-2 words in Stage 2's order as slices (word_off, word_len; at most INFX_MAX_QUERY_TOKENS) of
 *                                      `text` (at most INFX_MAX_QUERY_CHARS units); any output may be NULL
 *   infx_engine_highlight_rows         query qi's rows as returned (after Filter, SortBy and collapsing), each row hl_row_u16(term stride, snippet stride)
 *                                      uint16 in the layout of csrc/highlight.h; returns the rows written (at most cap_u16 / row size), -1 on error
 *   infx_engine_last_highlight_stats   highlighting queries and k_highlight launches of the session's last search: (k, 1), or (0, 0) without
 *   infx_engine_last_highlight_timings k_highlight's duration in that search (HIP events on its stream) and the bytes of rows it downloaded
 *   infx_engine_document_text          the stored text of document `document_index` (internal index): returns its length in UTF-16 units and copies at most
 *                                      cap of them, -1 on error */
#define INFX_HIGHLIGHT_MIN_CHARS 16
#define INFX_HIGHLIGHT_MAX_CHARS 512
#define INFX_HIGHLIGHT_MAX_SPANS 64
int32_t infx_engine_set_query_highlight(infx_session* s, uint32_t nq, const int32_t* chars /* 0: none */, int32_t* out_status /* nq, may be NULL */);
int32_t infx_engine_highlight_query(infx_session* s, uint32_t qi, int32_t* rows, int32_t* term_stride, int32_t* snippet_stride, int32_t* long_query,
                                    uint16_t* text, int32_t* text_len, uint16_t* word_off, uint16_t* word_len, int32_t* words);
int32_t infx_engine_highlight_rows(infx_session* s, uint32_t qi, uint16_t* out, int64_t cap_u16); /* rows written, -1 on error */
int32_t infx_engine_last_highlight_stats(infx_session* s, uint32_t* queries, uint32_t* launches);
int32_t infx_engine_last_highlight_timings(infx_session* s, float* ms, uint64_t* bytes);
int64_t infx_engine_document_text(infx_engine* e, int64_t document_index, uint16_t* out, int64_t cap);
/* ---- facets of the documents a filter accepts (not in the reference: the facet side of Query.pre_filter) --------------------------------------------------
 * The facets of an Infiscript expression P: the value counts of every facetable column (the first INFX_MAX_FACET_COLS) over the documents that are not Deleted
 * and whose OWN fields P accepts — per document, as NumberOfDocumentsInFilter counts and as the pre-filter masks are built, not through the key's first live
 * document.  Downstream of the counts they are infx_engine_facets_all's: null and empty values dropped, count descending then value ascending, at most 100
 * values per field.  The total of P is the number of those documents (= infx_engine_last_in_prefilter of a query with pre-filter P).
 * infx_engine_facets_filtered answers k expressions at once.  Answers are cached per expression in the engine (shared by its sessions, at most 256, least
 * recently used first out) for one mask epoch: deletions, restores, infx_engine_add_column and indexing invalidate them exactly as they invalidate the
 * pre-filter masks.  Only the distinct expressions the cache is missing go to the device, INFX_MAX_PREFILTERS (16) per infx_facets_filtered call: one pass
 * over the columns evaluates them all and counts every column.  An expression is refused ON ITS OWN — out_status[i], message from
 * infx_engine_facets_filtered_error, the other expressions unaffected — for a syntax error (INFX_EINVAL) or MATCHES (INFX_EUNSUPPORTED); the call itself then
 * still returns INFX_OK.  INFX_EHIP on an engine without a GPU.  Works on a sharded engine without a collective (every rank holds the whole columns and the
 * global Deleted flags, and returns the same answer).
 * Readers, for expression `which` of the session's last call: infx_engine_facets_filtered_column gives the k-th facet column (k <
 * infx_engine_facets_filtered_column_count) as infx_engine_facets_all_column does, -1 for a refused expression; infx_engine_facets_filtered_total the total
 * (returning the expression's status).  infx_engine_last_facets_filtered_stats: expressions counted on the device, expressions taken from the cache, and
 * k_facets_filtered launches of the session's last call. */
int32_t infx_engine_facets_filtered(infx_session* s, uint32_t k, const char* const* exprs, int32_t* out_status /* k, may be NULL */);
int32_t infx_engine_facets_filtered_column_count(infx_session* s);
int32_t infx_engine_facets_filtered_column(infx_session* s, uint32_t which, uint32_t k, int32_t* col, uint32_t* codes, uint32_t* counts, int32_t cap);
int32_t infx_engine_facets_filtered_total(infx_session* s, uint32_t which, uint32_t* total);
int32_t infx_engine_facets_filtered_error(infx_session* s, uint32_t which, char* out, int32_t cap);
int32_t infx_engine_last_facets_filtered_stats(infx_session* s, uint32_t* counted, uint32_t* cached, uint32_t* launches);
/* ---- list_documents: a filter's documents in the order of a field, by page (not in the reference: the semantics below are this project's) ---------------
 * Request i lists the SET of documents that are not Deleted and whose OWN fields its Infiscript `filter` accepts — per document, exactly the documents
 * infx_engine_last_in_prefilter and infx_engine_facets_filtered_total count; filter = NULL: every live document; duplicate keys are not collapsed — in the
 * ORDER (k(d), d): d the internal document index, k(d) = 1 + the sort rank of the document's value in field `order_by` (the ranks of Query.SortBy: long
 * numerically; double with NaN lowest, all NaNs equal, -0 == +0; strings OrdinalIgnoreCase then ordinal), mirrored (number of distinct values + 1 - k) when
 * `ascending` is 0, a constant when order_by = NULL (index order).  Ties go by ascending index in BOTH directions, so the order is total: pages never overlap
 * or skip, and any page equals the slice [offset, offset + limit) of the whole order.  1 <= limit <= 1024 (INFX_POST_MAX_ROWS, whatever max_post_rows is);
 * 0 <= offset < 2^31, a deep offset costs what offset 0 costs; offset >= total: an empty page with the total, no error.
 * A request is refused ON ITS OWN (out_status[i], message from infx_engine_list_error, the others unaffected): a syntax error, an unknown order_by field or
 * a limit / offset out of range INFX_EINVAL, MATCHES INFX_EUNSUPPORTED; the call itself then returns INFX_OK.  At most INFX_MAX_PREFILTERS (16) requests
 * (INFX_ECAPACITY): one mask slot per distinct filter.  INFX_EHIP on an engine without a GPU (no CPU fallback).  The masks are the session's pre-filter masks:
 * same slots, same least-recently-used rule, same epoch (deletions, restores, infx_engine_add_column and indexing invalidate them), and the ones a call is
 * missing are built in ONE launch in front of it; a column's sort rank is built on its first use.  Nothing else is cached.  Works on a sharded engine without
 * a collective (whole columns and global Deleted flags on every rank).
 * Readers, for request `which` of the session's last call: infx_engine_list_rows copies up to cap rows (DocumentKey, internal document, code of the
 * order_by column: its text through infx_engine_column_value) and returns the page's row count, -1 for a refused request or bad arguments;
 * infx_engine_list_total the size of the set (returning the request's status); infx_engine_list_error the refusal's message (its length; -1 out of range).
 * infx_engine_last_list_stats: masks built and reused, histogram passes and kernel launches of the session's last call.
 * infx_engine_set_list_digit_bits: the width of a radix-select digit on this session, 4 .. 11 (default 11) — a tuning knob. */
typedef struct infx_list_request { const char* filter; const char* order_by; int32_t ascending; uint32_t offset; uint32_t limit; } infx_list_request;
int32_t infx_engine_list_documents(infx_session* s, uint32_t nreq, const infx_list_request* reqs, int32_t* out_status /* nreq, may be NULL */);
int32_t infx_engine_list_rows(infx_session* s, uint32_t which, int64_t* keys, int32_t* docs, uint32_t* codes, int32_t cap);
int32_t infx_engine_list_total(infx_session* s, uint32_t which, uint32_t* total);
int32_t infx_engine_list_error(infx_session* s, uint32_t which, char* out, int32_t cap);
int32_t infx_engine_last_list_stats(infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* hist_passes, uint32_t* launches);
int32_t infx_engine_set_list_digit_bits(infx_session* s, int32_t bits);
/* ---- range_facets: bucket counts and min / max of a numeric field over a filter (not in the reference: the semantics below are this project's) ----------
 * Request i asks, over the SET of infx_engine_list_documents — every document that is not Deleted and whose OWN fields its Infiscript `filter` accepts;
 * filter = NULL: every live document; duplicate keys are documents of their own — for the values v of `field`, an int64 or a double column:
 *   counts[j]  documents with e_j <= v < e_(j+1): every bucket is half-open, the last included        below  documents with v < e_0
 *   above      documents with v >= e_B                                                                  nan    documents whose value is a NaN (double columns)
 *   total      the size of the set, whatever the edges: nan + below + sum(counts) + above == total
 *   min, max   the smallest and largest value of the set that is not a NaN (none: kind 0); -0.0 and +0.0 compare equal, either may come back
 * Values compare as Query.SortBy compares them (long numerically; double numerically with -0 == +0).  A NaN value is in no bucket and not in min / max.
 * EDGES: nedges = 2 .. 257 (1 .. 256 buckets), strictly increasing under that comparison (so -0.0, 0.0 is not), no NaN, +-inf allowed on a double column.
 * An int64 column reads edges_i (NULL: INFX_EINVAL, "integer column needs integer edges"), a double column reads edges_d.
 * No sums or means (per bucket: infx_engine_bucket_stats) and no percentiles (a percentile is infx_engine_list_documents at offset p * total, limit 1); nothing is cached but the masks.
 * A request is refused ON ITS OWN (out_status[i], message from infx_engine_range_error, the others answered): a syntax error, an unknown field, a string
 * column or bad edges INFX_EINVAL, MATCHES INFX_EUNSUPPORTED; the call itself then returns INFX_OK.  At most INFX_MAX_PREFILTERS (16) requests
 * (INFX_ECAPACITY).  INFX_EHIP on an engine without a GPU (no CPU fallback), the field and edge refusals already in out_status; a call that failed as a
 * whole leaves nothing for the readers.  The masks are the session's pre-filter masks (slots, least-recently-used rule, epoch and statistics of
 * infx_engine_list_documents; the ones a call is missing are built in ONE launch in front of it); the column's sort rank is built on its first use; ONE
 * k_range_counts launch counts all requests of the call.  Works on a sharded engine without a collective.
 * Readers, for request `which` of the session's last call: infx_engine_range_counts copies up to cap bucket counts and below / above / nan and returns the
 * number of buckets (-1 for a refused request or bad arguments); infx_engine_range_total the size of the set (returning the request's status);
 * infx_engine_range_minmax *kind = 1 with lo_i / hi_i, 2 with lo_d / hi_d, 0 when the set holds no value that is not a NaN; infx_engine_range_error the
 * refusal's message (its length; -1 out of range).  infx_engine_last_range_stats: masks built and reused and k_range_counts launches of the last call. */
typedef struct infx_range_request { const char* filter; const char* field; uint32_t nedges; const int64_t* edges_i; const double* edges_d; } infx_range_request;
int32_t infx_engine_range_facets(infx_session* s, uint32_t nreq, const infx_range_request* reqs, int32_t* out_status /* nreq, may be NULL */);
int32_t infx_engine_range_counts(infx_session* s, uint32_t which, uint32_t* counts, int32_t cap, uint32_t* below, uint32_t* above, uint32_t* nan);
int32_t infx_engine_range_total(infx_session* s, uint32_t which, uint32_t* total);
int32_t infx_engine_range_minmax(infx_session* s, uint32_t which, int32_t* kind, int64_t* lo_i, int64_t* hi_i, double* lo_d, double* hi_d);
int32_t infx_engine_range_error(infx_session* s, uint32_t which, char* out, int32_t cap);
int32_t infx_engine_last_range_stats(infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* launches);
/* ---- field_stats: counts, min / max and the EXACT sum and mean of a numeric field over a filter, whole or per group (not in the reference: the semantics
 * below are this project's) ----
 * Request i asks, over the SET of infx_engine_list_documents — every document that is not Deleted and whose OWN fields its Infiscript `filter` accepts;
 * filter = NULL: every live document; duplicate keys are documents of their own — for the values v of `field`, an int64 or a double column:
 *   nan        members whose value is a NaN; they appear in no other figure            count   the other members; count + nan is the size of the set
 *   min, max   the smallest and largest value that is not a NaN, as infx_engine_range_minmax returns them (valid when count > 0)
 *   sum        kind 1 (int64 column): the exact sum as the 128-bit two's complement integer sum_hi : sum_lo, and rounded once in sum_d
 *              kind 2 (double column): sum_d = the exact real sum of the finite values rounded ONCE to nearest-even (what math.fsum returns); beyond the
 *              double range +-inf; with +inf members and no -inf member +inf, the mirror case -inf, both a NaN; a zero sum is +0.0; an empty set 0
 *   mean       valid when count > 0: the exact sum divided by count, rounded once, for both kinds; +-inf / NaN as the sum
 * and, with `group_by` (any column of any kind, facetable or not, of at most INFX_STATS_MAX_GROUPS = 4096 distinct values; it may be `field` itself), the
 * same figures for every distinct value of group_by that has a member: ALL such groups (no cut at 100), members descending, then the group column's facet
 * tie order ascending.  The groups' count and nan add up to the whole's; on an int64 column so do the sums.
 * The sums do not depend on the order of the additions: the device adds integers only (DESIGN.md "field_stats"), so every run, session, stream and rank
 * returns the same bytes.  No variance, distinct counts or top-N cut (percentiles: infx_engine_field_quantiles); nothing is cached but the masks.
 * A request is refused ON ITS OWN (out_status[i], message from infx_engine_field_stats_error, the others answered): a syntax error, a missing or unknown
 * field, an unknown group_by, a string field, a group_by of more than 4096 values, or a double column whose finite values span more than 128 binary digits
 * (it cannot be summed exactly) INFX_EINVAL, MATCHES INFX_EUNSUPPORTED; the call itself then returns INFX_OK.  At most INFX_MAX_PREFILTERS (16) requests
 * (INFX_ECAPACITY).  INFX_EHIP on an engine without a GPU (no CPU fallback), every refusal but the filter's already in out_status; a call that failed as
 * a whole leaves nothing for the readers.  The masks are the session's pre-filter masks (slots, least-recently-used rule, epoch and statistics of
 * infx_engine_list_documents); the field's sort rank and value table are built on first use and dropped when infx_engine_add_column replaces the column;
 * ONE k_field_stats launch answers all requests of the call.  Works on a sharded engine without a collective.
 * Readers, for request `which` of the session's last call: infx_engine_field_stats_whole the whole's figures (returning the request's status);
 * infx_engine_field_stats_groups copies up to cap groups in the order above — codes[g] the group's code in column *group_col (-1 without group_by; its
 * text through infx_engine_column_value), figures[g] its figures — and returns the number of groups (-1 for a refused request or bad arguments);
 * infx_engine_field_stats_total the size of the set (returning the request's status); infx_engine_field_stats_error the refusal's message (its length; -1
 * out of range).  infx_engine_last_field_stats_stats: masks built and reused and k_field_stats launches of the last call. */
typedef struct infx_stats_request { const char* filter; const char* field; const char* group_by; } infx_stats_request;
typedef struct infx_stats_figures { uint32_t count; uint32_t nan; int32_t kind; int32_t reserved; int64_t min_i; int64_t max_i; double min_d; double max_d; double sum_d; uint64_t sum_lo; int64_t sum_hi; double mean; } infx_stats_figures;
int32_t infx_engine_field_stats(infx_session* s, uint32_t nreq, const infx_stats_request* reqs, int32_t* out_status /* nreq, may be NULL */);
int32_t infx_engine_field_stats_whole(infx_session* s, uint32_t which, infx_stats_figures* out);
int32_t infx_engine_field_stats_groups(infx_session* s, uint32_t which, int32_t* group_col, uint32_t* codes, infx_stats_figures* figures, int32_t cap);
int32_t infx_engine_field_stats_total(infx_session* s, uint32_t which, uint32_t* total);
int32_t infx_engine_field_stats_error(infx_session* s, uint32_t which, char* out, int32_t cap);
int32_t infx_engine_last_field_stats_stats(infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* launches);
/* ---- bucket_stats: the EXACT sums and means of a numeric field per range bucket of a second numeric field over a filter (not in the reference: the
 * semantics below are this project's) ----
 * Request i asks, over the SET of infx_engine_list_documents — every document that is not Deleted and whose OWN fields its Infiscript `filter` accepts;
 * filter = NULL: every live document — for infx_engine_field_stats' figures of `field` over the members of every bucket of `bucket_by`:
 *   bucket_by, edges   infx_engine_range_facets' field and edges, under the same rules: an int64 or a double column; nedges = 2 .. 257 strictly increasing edges
 *              e_0 < .. < e_B as Query.SortBy compares values, no NaN, +-inf allowed on a double column; an int64 column reads edges_i, a double column edges_d
 *   field      infx_engine_field_stats' field: an int64 or a double column whose finite values span at most 128 binary digits; it may be bucket_by itself
 *   rows       B + 3 of them, in the order [below | B buckets | above | nan]: the members whose bucket_by value is below e_0, in [e_j, e_(j+1)), at or above
 *              e_B, or a NaN.  Per row its size (its members) and the six figures of `field` over them — count, nan, min, max, sum, mean exactly as
 *              infx_engine_field_stats defines and computes them (the same functions); size == count + nan; an empty row reads as infx_engine_field_stats
 *              on an empty set
 *   whole      the figures of `field` over the whole set, equal figure for figure to infx_engine_field_stats(filter, field): the host adds the rows' slots
 *              as integers, as a grouped infx_engine_field_stats does;  total  the size of the set
 * The rows' sizes are infx_engine_range_facets' counts, below, above and nan for the same filter, field = bucket_by and edges; nan.size + below.size + the
 * buckets' sizes + above.size == total == whole.count + whole.nan; the rows' count and nan add up to the whole's, and on an int64 `field` so do the sums.
 * The device adds integers only (DESIGN.md "bucket_stats"), so every run, session, stream, placement and rank returns the same bytes.  Left out on purpose:
 * a group_by beside the buckets, quantiles per bucket, automatic edges, a Query option; nothing is cached but the masks.
 * A request is refused ON ITS OWN (out_status[i], message from infx_engine_bucket_stats_error, the others answered): a syntax error, a missing, unknown or
 * string field, a field that cannot be summed exactly, a missing, unknown or string bucket_by or bad edges INFX_EINVAL (the messages of
 * infx_engine_field_stats and infx_engine_range_facets, naming bucket_stats), MATCHES INFX_EUNSUPPORTED; the call itself then returns INFX_OK.  At most
 * INFX_MAX_PREFILTERS (16) requests (INFX_ECAPACITY).  INFX_EHIP on an engine without a GPU (no CPU fallback), every refusal but the filter's already in
 * out_status; a call that failed as a whole leaves nothing for the readers.  The masks are the session's pre-filter masks; both columns' sort ranks and the
 * field's value table are built on first use and dropped when infx_engine_add_column replaces the column; ONE k_bucket_stats launch answers all requests of
 * the call.  Works on a sharded engine without a collective.
 * Readers, for request `which` of the session's last call: infx_engine_bucket_stats_rows copies up to cap rows in the order above — sizes[k] and figures[k]
 * of row k — and returns the number of rows, B + 3 (-1 for a refused request or bad arguments); infx_engine_bucket_stats_whole the whole's figures and
 * infx_engine_bucket_stats_total the size of the set (both returning the request's status); infx_engine_bucket_stats_error the refusal's message (its
 * length; -1 out of range).  infx_engine_last_bucket_stats_stats: masks built and reused and k_bucket_stats launches of the last call;
 * infx_engine_last_bucket_stats_placement: its requests whose slots lay in a workgroup's LDS, in a CU's whole LDS and in global memory
 * (infx_last_bucket_stats_info). */
typedef struct infx_bucket_stats_request { const char* filter; const char* field; const char* bucket_by; uint32_t nedges; const int64_t* edges_i; const double* edges_d; } infx_bucket_stats_request;
int32_t infx_engine_bucket_stats(infx_session* s, uint32_t nreq, const infx_bucket_stats_request* reqs, int32_t* out_status /* nreq, may be NULL */);
int32_t infx_engine_bucket_stats_rows(infx_session* s, uint32_t which, uint32_t* sizes, infx_stats_figures* figures, int32_t cap);
int32_t infx_engine_bucket_stats_whole(infx_session* s, uint32_t which, infx_stats_figures* out);
int32_t infx_engine_bucket_stats_total(infx_session* s, uint32_t which, uint32_t* total);
int32_t infx_engine_bucket_stats_error(infx_session* s, uint32_t which, char* out, int32_t cap);
int32_t infx_engine_last_bucket_stats_stats(infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* launches);
int32_t infx_engine_last_bucket_stats_placement(infx_session* s, uint32_t* small_lds, uint32_t* big_lds, uint32_t* in_global);
/* ---- field_quantiles: exact medians and percentiles of a numeric field over a filter, whole and per group (not in the reference: the semantics below are
 * this project's) ----
 * Request i asks, over the SET of infx_engine_field_stats (what infx_engine_list_total and infx_engine_field_stats_total count), for nq quantiles q[0 .. nq)
 * of `field`, an int64 or a double column — 1 <= nq <= INFX_QUANT_MAX (16), every q[t] a number in [0, 1], in any order, duplicates allowed:
 *   nan        members whose value is a NaN; they are in no quantile                    count   the other members; count + nan is the size of the set
 *   value t    the value at 0-based position floor((count - 1) * q[t]) of the non-NaN members in ascending order of infx_engine_set_sort's comparison —
 *              the product ONE IEEE double multiplication: the element numpy.quantile(method="lower") picks.  No interpolation: always a value some
 *              member has, returned as min / max are (through the rank's lowest code; v_i for kind 1, v_d for kind 2); +-inf are ordinary values.  Valid
 *              when count > 0.  q = 0 is infx_engine_field_stats' min, q = 1 its max; infx_engine_list_documents at order_by = field, ascending,
 *              offset = nan + position, limit = 1 lists a document of that value (NaNs hold the lowest ranks).
 * and, with `group_by` (infx_engine_field_stats' rule: any column of at most 4096 distinct values, `field` itself included), the same figures for every
 * distinct value of group_by that has a member, each at the positions of its OWN count, in infx_engine_field_stats' order of groups.
 * Exact and deterministic: the device selects on sort ranks with integer adds (DESIGN.md "field_quantiles"), so every run, session, stream and rank returns
 * the same bytes.  Nothing is cached but the masks.
 * A request is refused ON ITS OWN (out_status[i], message from infx_engine_field_quantiles_error, the others answered): a syntax error, a missing, unknown
 * or string field, an unknown group_by or one of more than 4096 values, nq = 0 or q = NULL, nq > 16, a q[t] outside [0, 1] or a NaN INFX_EINVAL, MATCHES
 * INFX_EUNSUPPORTED; the call itself then returns INFX_OK.  At most INFX_MAX_PREFILTERS (16) requests (INFX_ECAPACITY).  INFX_EHIP on an engine without a
 * GPU (no CPU fallback), every refusal but the filter's already in out_status; a call that failed as a whole leaves nothing for the readers.  The masks are
 * the session's pre-filter masks; every pass of the select is one k_quant_hist and one k_quant_pick launch for all requests of the call.  Works on a
 * sharded engine without a collective.
 * Readers, for request `which` of the session's last call: infx_engine_field_quantiles_whole the whole's figures (returning the request's status);
 * infx_engine_field_quantiles_groups copies up to cap groups — codes[g] the group's code in column *group_col (-1 without group_by), figures[g] its
 * figures — and returns the number of groups (-1 for a refused request or bad arguments); infx_engine_field_quantiles_total the size of the set (returning
 * the request's status); infx_engine_field_quantiles_error the refusal's message (its length; -1 out of range).
 * infx_engine_last_field_quantiles_stats: masks built and reused, histogram passes (k_quant_hist launches) and kernel launches of the last call.
 * infx_engine_last_field_quantiles_placement: the digit width the last call chose (the cap under which every request's width lies) and how many of its
 * (request, pass) pairs had their bins in LDS / in global memory (infx_last_field_quantiles_info).
 * infx_engine_set_quantile_digit_bits: the width of the select's radix digit on this session, 4 .. 11, or 0 (the default): the engine chooses per call.  It
 * changes the number of passes, never an answer. */
typedef struct infx_quantile_request { const char* filter; const char* field; const char* group_by; const double* q; uint32_t nq; } infx_quantile_request;
typedef struct infx_quantile_figures { uint32_t count; uint32_t nan; int32_t kind; uint32_t nq; int64_t v_i[16]; double v_d[16]; } infx_quantile_figures;
int32_t infx_engine_field_quantiles(infx_session* s, uint32_t nreq, const infx_quantile_request* reqs, int32_t* out_status /* nreq, may be NULL */);
int32_t infx_engine_field_quantiles_whole(infx_session* s, uint32_t which, infx_quantile_figures* out);
int32_t infx_engine_field_quantiles_groups(infx_session* s, uint32_t which, int32_t* group_col, uint32_t* codes, infx_quantile_figures* figures, int32_t cap);
int32_t infx_engine_field_quantiles_total(infx_session* s, uint32_t which, uint32_t* total);
int32_t infx_engine_field_quantiles_error(infx_session* s, uint32_t which, char* out, int32_t cap);
int32_t infx_engine_last_field_quantiles_stats(infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* hist_passes, uint32_t* launches);
int32_t infx_engine_last_field_quantiles_placement(infx_session* s, uint32_t* digit_bits, uint32_t* lds_rows, uint32_t* global_rows);
int32_t infx_engine_set_quantile_digit_bits(infx_session* s, int32_t bits);
/* ---- list_groups: one row per value of a field, in the order of a field, by page (not in the reference: the semantics below are this project's) -----------
 * Request i lists, over the SET of infx_engine_list_documents — every document that is not Deleted and whose OWN fields its Infiscript `filter` accepts;
 * filter = NULL: every live document; duplicate keys are documents of their own — and in its ORDER (k(d), d) for `order_by` and `ascending` (ties by ascending
 * index in both directions; order_by = NULL: index order):
 *   GROUP   one dictionary code of field `group_by`, exactly as infx_engine_field_stats forms and names groups (the text of infx_engine_column_value): any
 *           column of any kind, facetable or not, of any number of distinct values; it may be order_by itself
 *   HEAD    of a group with a member: its member that comes first in the ORDER — "the cheapest offer of every product", "the newest post of every author"
 *   ANSWER  the rows at [offset, min(offset + limit, total_groups)) of the heads in the ORDER, i.e. infx_engine_list_documents over the SET restricted to
 *           the heads: pages never overlap or skip.  Per row the DocumentKey, the internal document, the code of the order_by column, the code of the
 *           group_by column and the number of members of that group in the SET
 *   total_groups   the number of groups with a member: the exact distinct count of group_by over the filter       total   the size of the SET
 * 1 <= limit <= 1024, 0 <= offset < 2^31; offset >= total_groups: an empty page with both totals, no error.  No more than one row per group, no order by
 * size; nothing is cached but the masks.
 * A request is refused ON ITS OWN (out_status[i], message from infx_engine_group_list_error, the others answered): a syntax error, a missing or unknown
 * group_by, an unknown order_by or a limit / offset out of range INFX_EINVAL, MATCHES INFX_EUNSUPPORTED; the call itself then returns INFX_OK.  At most
 * INFX_MAX_PREFILTERS (16) requests (INFX_ECAPACITY).  INFX_EHIP on an engine without a GPU (no CPU fallback), every refusal but the filter's already in
 * out_status; a call that failed as a whole leaves nothing for the readers.  The masks are the session's pre-filter masks (slots, least-recently-used rule,
 * epoch and statistics of infx_engine_list_documents; the ones a call is missing are built in ONE launch in front of it); order_by's sort rank is built on
 * its first use.  Requests that share filter, group_by, order_by and direction — the pages of one listing — share one head pass.  Exact and deterministic:
 * the same bytes from any session, stream and rank.  Works on a sharded engine without a collective.
 * Readers, for request `which` of the session's last call: infx_engine_group_list_rows copies up to cap rows and returns the page's row count (-1 for a
 * refused request or bad arguments); infx_engine_group_list_totals both totals (returning the request's status); infx_engine_group_list_error the refusal's
 * message (its length; -1 out of range).  infx_engine_last_group_list_stats: masks built and reused, head passes, histogram passes and kernel launches of
 * the session's last call.  infx_engine_set_list_digit_bits governs the pages' select here too. */
typedef struct infx_group_list_request { const char* filter; const char* group_by; const char* order_by; int32_t ascending; uint32_t offset; uint32_t limit; } infx_group_list_request;
int32_t infx_engine_list_groups(infx_session* s, uint32_t nreq, const infx_group_list_request* reqs, int32_t* out_status /* nreq, may be NULL */);
int32_t infx_engine_group_list_rows(infx_session* s, uint32_t which, int64_t* keys, int32_t* docs, uint32_t* codes, uint32_t* group_codes, uint32_t* sizes, int32_t cap);
int32_t infx_engine_group_list_totals(infx_session* s, uint32_t which, uint32_t* total_groups, uint32_t* total);
int32_t infx_engine_group_list_error(infx_session* s, uint32_t which, char* out, int32_t cap);
int32_t infx_engine_last_group_list_stats(infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* head_passes, uint32_t* hist_passes, uint32_t* launches);
/* ---- list_group_members: the first N documents of every group, by page (not in the reference: the semantics below are this project's) --------------------
 * Request i is infx_engine_list_groups' request plus `per_group`.  Its SET, ORDER, GROUPS and HEADS are that call's; its ROWS are exactly the rows of
 * infx_engine_list_groups for the same filter, group_by, order_by, ascending, offset and limit, in the same order — by each group's head — with the same
 * sizes, total_groups and total.  Every row carries the MEMBERS of its group: the first min(per_group, size) members of the group in the ORDER (key, internal
 * index; ties by ascending index in both directions; duplicate DocumentKeys are members of their own), the head first.  "The three cheapest offers of every
 * product family, page 7" in one call instead of one listing per row: the members are kept in the walk that counts the groups' sizes.
 * 1 <= per_group <= 16, 1 <= limit <= 1024 and limit * per_group <= 4096 (INFX_GROUP_MEMBERS_MAX); the other limits and every refusal are
 * infx_engine_list_groups', per request (out_status[i], message from infx_engine_group_members_error).  At most 16 requests (INFX_ECAPACITY); INFX_EHIP on an
 * engine without a GPU, every refusal but the filter's already in out_status.  Masks, sort ranks and the sharing of head passes as there.  The members are
 * ordered by one field only, the groups' own; nothing is cached but the masks.  Exact and deterministic: the same bytes from any session, stream and rank.
 * Readers, for request `which` of the session's last call.  infx_engine_group_members_rows: up to cap rows — the group's code, its size and the number of
 * members it carries — returning the page's row count (-1 for a refused request or bad arguments).  infx_engine_group_members_members: the members of ALL
 * rows, row after row (row r's are the member_counts[r] entries behind those of the rows before it): up to cap members' DocumentKeys, internal documents and
 * codes of the order_by column (0 without one), returning the page's member count (-1 as above) — two readers, because the rows are at most 1024 and
 * the members at most 4096.  infx_engine_group_members_totals, _error and infx_engine_last_group_members_stats (masks built and reused, head passes,
 * histogram passes, member walks, kernel launches) as infx_engine_list_groups' readers. */
typedef struct infx_group_members_request { const char* filter; const char* group_by; const char* order_by; int32_t ascending; uint32_t offset; uint32_t limit; uint32_t per_group; } infx_group_members_request;
int32_t infx_engine_list_group_members(infx_session* s, uint32_t nreq, const infx_group_members_request* reqs, int32_t* out_status /* nreq, may be NULL */);
int32_t infx_engine_group_members_rows(infx_session* s, uint32_t which, uint32_t* group_codes, uint32_t* sizes, uint32_t* member_counts, int32_t cap);
int32_t infx_engine_group_members_members(infx_session* s, uint32_t which, int64_t* keys, int32_t* docs, uint32_t* codes, int32_t cap);
int32_t infx_engine_group_members_totals(infx_session* s, uint32_t which, uint32_t* total_groups, uint32_t* total);
int32_t infx_engine_group_members_error(infx_session* s, uint32_t which, char* out, int32_t cap);
int32_t infx_engine_last_group_members_stats(infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* head_passes, uint32_t* hist_passes, uint32_t* member_walks, uint32_t* launches);
/* ---- top_groups: a field's groups ranked by size, count, min, max, sum or mean, by page (not in the reference: the semantics below are this project's) ------
 * Request i ranks, over the SET of infx_engine_list_documents — every document that is not Deleted and whose OWN fields its Infiscript `filter` accepts;
 * filter = NULL: every live document:
 *   GROUP   one dictionary code of field `group_by`, formed and named exactly as in infx_engine_field_stats and infx_engine_list_groups: any column of any
 *           kind and ANY number of distinct values, a unique column and `field` itself included
 *   FIELD   an int64 or a double column infx_engine_field_stats can sum (at most 128 binary digits); NULL only with by = "size"
 *   FIGURE  of a group, by `by`: "size" its members in the SET; "count" those whose value is not a NaN; "min" / "max" infx_stats_figures' min / max, compared
 *           by the column's sort rank (-0.0 and 0.0 tie); "sum" its sum — an int column's exact integer compared exactly, a double column's exact real sum
 *           rounded once compared as a double, -inf < finite < +inf; "mean" its mean as a double.  A group whose figure is none or a NaN — min / max / mean
 *           with count == 0, a sum or mean over both infinities — has NO figure
 *   ORDER   the groups with a figure by the figure, ascending or descending; then, in BOTH directions, the groups without one; every tie by the group
 *           column's facet tie order (infx_engine_field_stats' order of equal groups), ascending in both directions.  The order is total
 *   ANSWER  the rows at [offset, min(offset + limit, total_groups)): per row the group's code, its members and — with a field — the figures
 *           infx_engine_field_stats returns for that group, from the same functions; only groups with a member are rows
 *   total_groups   the number of groups with a member (infx_engine_group_list_totals')       total   the size of the SET
 * 1 <= limit <= 1024, 0 <= offset < 2^31; offset >= total_groups: an empty page with both totals, no error.  Nothing is cached but the masks.
 * A request is refused ON ITS OWN (out_status[i], message from infx_engine_top_groups_error, the others answered): a syntax error, a missing or unknown
 * group_by, an unknown `by`, a `by` other than "size" without a field, an unknown or string field, a field that is not exactly summable or a limit / offset
 * out of range INFX_EINVAL, MATCHES INFX_EUNSUPPORTED; the call itself then returns INFX_OK.  At most INFX_MAX_PREFILTERS (16) requests (INFX_ECAPACITY).
 * INFX_EHIP on an engine without a GPU (no CPU fallback), every refusal but the filter's already in out_status; a call that failed as a whole leaves nothing
 * for the readers.  The masks are the session's pre-filter masks, as for infx_engine_list_documents.  Requests that share filter, field and group_by — pages,
 * directions and `by`s of one table — share one accumulate pass.  Exact and deterministic: integer adds, minima and maxima only; the same bytes from any
 * session, stream and rank.  Works on a sharded engine without a collective.
 * Readers, for request `which` of the session's last call: infx_engine_top_groups_rows copies up to cap rows (figures[r].kind is 0 throughout a request
 * without a field) and returns the page's row count (-1 for a refused request or bad arguments); infx_engine_top_groups_totals both totals (returning the
 * request's status); infx_engine_top_groups_error the refusal's message (its length; -1 out of range).  infx_engine_last_top_groups_stats: masks built and
 * reused, accumulate passes, select passes (histogram launches) and kernel launches of the session's last call; infx_engine_last_top_groups_placement: the
 * tables it accumulated in a workgroup's LDS, in a CU's whole LDS and in global memory.  infx_engine_set_list_digit_bits governs the select here too. */
typedef struct infx_top_request { const char* filter; const char* group_by; const char* by; const char* field; int32_t ascending; uint32_t offset; uint32_t limit; } infx_top_request;
int32_t infx_engine_top_groups(infx_session* s, uint32_t nreq, const infx_top_request* reqs, int32_t* out_status /* nreq, may be NULL */);
int32_t infx_engine_top_groups_rows(infx_session* s, uint32_t which, int32_t* group_col, uint32_t* codes, uint32_t* sizes, infx_stats_figures* figures, int32_t cap);
int32_t infx_engine_top_groups_totals(infx_session* s, uint32_t which, uint32_t* total_groups, uint32_t* total);
int32_t infx_engine_top_groups_error(infx_session* s, uint32_t which, char* out, int32_t cap);
int32_t infx_engine_last_top_groups_stats(infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* accumulate_passes, uint32_t* select_passes, uint32_t* launches);
int32_t infx_engine_last_top_groups_placement(infx_session* s, uint32_t* small_lds, uint32_t* big_lds, uint32_t* in_global);
/* ---- field_distinct: the exact number of distinct values of a field, whole and per group (not in the reference: the semantics below are this project's) ------
 * Request i counts, over the SET of infx_engine_list_documents — every document that is not Deleted and whose OWN fields its Infiscript `filter` accepts;
 * filter = NULL: every live document:
 *   VALUE   one dictionary code of `field`, exactly the groups infx_engine_list_groups forms of it: `distinct` of a request without group_by IS that call's
 *           total_groups.  Codes are given by the stored bytes — an int64 by its number, a string by its bytes, a double by its BIT PATTERN: -0.0 and 0.0 are
 *           two values, a NaN is a value, and NaNs of different payloads are different values
 *   FIELD   any column of any kind and any number of values, a string column and a unique column included
 *   GROUP   with `group_by` (any column of at most INFX_STATS_MAX_GROUPS = 4096 values, checked as infx_engine_field_stats checks it; it may be `field`
 *           itself — every group then holds one value): per group with a member its members (size) and the values of `field` among them (distinct), in
 *           infx_engine_field_stats' order of groups
 *   whole   distinct: the values of `field` in the SET, with or without group_by; size: the SET's size (also infx_engine_field_distinct_total)
 * A request is refused ON ITS OWN (out_status[i], message from infx_engine_field_distinct_error, the others answered): a syntax error, a missing or unknown
 * field, an unknown group_by or one of more than 4096 values INFX_EINVAL, MATCHES INFX_EUNSUPPORTED; the call itself then returns INFX_OK.  At most
 * INFX_MAX_PREFILTERS (16) requests (INFX_ECAPACITY).  INFX_EHIP on an engine without a GPU (no CPU fallback), every refusal but the filter's already in
 * out_status; a call that failed as a whole leaves nothing for the readers.  Nothing is cached but the masks, the session's pre-filter masks.  Requests that
 * share filter, field and group_by share one pass.  Exact and deterministic — bit ORs, compare-and-swap installs counted once and integer adds only: the same
 * bytes from any session, stream, placement and rank.  Works on a sharded engine without a collective.
 * Readers, for request `which` of the session's last call: _whole, _groups, _total and _error as infx_engine_field_stats'.
 * infx_engine_last_field_distinct_stats: masks built and reused, the passes that marked in LDS, in a global bitmap and in a hash set, and kernel launches of
 * the session's last call.  infx_engine_set_distinct_placement: where this session's passes mark — 0 automatic (default), 1 LDS, 2 global bitmap, 3 hash set;
 * a forced placement that does not fit falls to the next larger one.  For tests and measurements: the answer does not depend on it. */
typedef struct infx_distinct_request { const char* filter; const char* field; const char* group_by; } infx_distinct_request;
typedef struct infx_distinct_figures { uint32_t size; uint32_t distinct; } infx_distinct_figures;
int32_t infx_engine_field_distinct(infx_session* s, uint32_t nreq, const infx_distinct_request* reqs, int32_t* out_status /* nreq, may be NULL */);
int32_t infx_engine_field_distinct_whole(infx_session* s, uint32_t which, infx_distinct_figures* out);
int32_t infx_engine_field_distinct_groups(infx_session* s, uint32_t which, int32_t* group_col, uint32_t* codes, infx_distinct_figures* figures, int32_t cap);
int32_t infx_engine_field_distinct_total(infx_session* s, uint32_t which, uint32_t* total);
int32_t infx_engine_field_distinct_error(infx_session* s, uint32_t which, char* out, int32_t cap);
int32_t infx_engine_last_field_distinct_stats(infx_session* s, uint32_t* masks_built, uint32_t* masks_reused, uint32_t* lds_passes, uint32_t* bitmap_passes, uint32_t* hash_passes, uint32_t* launches);
int32_t infx_engine_set_distinct_placement(infx_session* s, int32_t mode);
int32_t infx_engine_set_filter_cache_limit(infx_engine* e, uint64_t limit);
int64_t infx_engine_filter_cache_size(infx_engine* e);
/* The infx_cov_query (CoverageEngine.PrepareQuery) the engine would hand to the device for this raw query text: lets a caller of the device ABI
 * (infx_stage2_batch) prepare Stage-2 inputs without the engine's search path. */
int32_t infx_engine_prepare_cov_query(infx_engine* e, const uint16_t* q, int32_t len, infx_cov_query* out);
int32_t infx_sizeof_cov_query(void);
/* the same for a query beyond the fast Stage-2 envelope (infx_engine_prepare_cov_query returns INFX_EUNSUPPORTED for it): the record of the long-query table
 * (infx_stage2_long_queries, include/infidex_hip.h) */
int32_t infx_engine_prepare_cov_query_long(infx_engine* e, const uint16_t* q, int32_t len, infx_cov_query_long* out);
int32_t infx_sizeof_cov_query_long(void);
int32_t infx_engine_effective_cpus(void);
/* Sharded planning — the PLAN EXCHANGE.  Every rank of a document-sharded job answers the same queries and holds the whole host index, and planning is a
 * pure function of (index, query text): rank r therefore plans queries [begin, end) of the coming batch only — text preparation and term lookups
 * (VectorModel.cs:376-420), the coverage query context (CoverageEngine.PrepareQuery, CoverageEngine.cs:61-126) and, when the dictionaries are NOT on the device,
 * the LD1 expansions and WordMatcher descriptors — the ranks exchange the serialised results (one all-gather of byte blobs on a transport of the caller's,
 * infidex_amd/sharded.py: a gloo group per pipeline session) and import each other's before infx_session_phase0, which then only runs what depends on
 * the batch as a whole or on this shard (expansion cache, fuzzy unions and their global df, idf / roles, list descriptors).  Per-rank host work per query
 * goes from the whole plan to 1/W of it plus the import.  collect returns the blob size (or -1) and keeps this rank's own slice, blob copies it out, import
 * takes a peer's blob (validated: everything in it that reaches the device is range-checked; a plan is only used for the text and depth it was made for).
 * Results are identical with or without the exchange. */
int64_t infx_session_prefetch_collect(infx_session* s, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, uint32_t begin, uint32_t end, int32_t depth);
int32_t infx_session_prefetch_blob(infx_session* s, uint8_t* out, int64_t cap);
int32_t infx_session_prefetch_import(infx_session* s, const uint8_t* blob, int64_t len);
int64_t infx_session_prefetch_pending(infx_session* s);        /* imported WordMatcher descriptor sets waiting for the next phase 0 */
int32_t infx_session_plan_exchange_stats(infx_session* s, uint32_t* out2 /* last phase 0: queries planned from the exchange (own slice + imported), of them imported */);
/* parity tooling, no device needed: a digest per query of everything the exchange carries for it, from the pending exchange entries where they match the text,
 * computed locally otherwise (*from_exchange counts the former); entries are not consumed */
int32_t infx_session_plan_digest(infx_session* s, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, int32_t depth, uint64_t* out, uint32_t* from_exchange);
/* Measurement hook (no device needed): single-threaded host planning cost of a batch by stage, microseconds per query:
 * out_us[0] plan_tokens, [1] of it LD1 walks, [2] plan_finish, [3] wm_collect, [4] prepare_cov_query, [5] plan_tokens_text (the exchangeable share of [0]),
 * [6] import of the batch's exchanged plans, [7] parsing them in phase 0 (replaces [5] + [4] for an imported query).  out_us holds 8 doubles. */
int32_t infx_engine_host_plan_profile(infx_engine* e, uint32_t nq, const uint16_t* q_arena, const uint64_t* q_offs, int32_t depth, double* out_us);
/* Entries of the LD1 expansion cache (least recently used, at most 1000: VectorModel.cs:42). */
int64_t infx_engine_fuzzy_cache_size(infx_engine* e);
/* Switches infx_engine_config.want_features at run time (the introspection buffers behind infx_engine_last_stage1 / _last_stage2). */
int32_t infx_engine_set_introspection(infx_engine* e, int32_t on);
int32_t infx_engine_normalize(const uint16_t* s, int32_t len, int32_t lower, uint16_t* out, int32_t cap);
int32_t infx_engine_device_handles(infx_engine* e, infx_index** idx, infx_stream** st);

#ifdef __cplusplus
}
#endif
#endif
