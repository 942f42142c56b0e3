// Query.collapse_by on the device: at most `keep` rows per group of a ranked list.  Not in the reference (DESIGN.md, "collapse_by").  Included by infidex_hip.hip.
//
// k_finalize writes the whole ranked list L of a collapsing query — up to `depth` rows with their documents — into the query's window of the stream's scratch
// (k_finalize_win below; truncation is decided there, on the uncollapsed list).  k_collapse, one workgroup per collapsing query, reads the window, keeps the rows
// whose rank within their group is below `keep`, and writes the first max_results of them into the query's rows of the batch buffers, where k_postfilter and
// k_postproc find them as they find any query's rows.  The arithmetic is collapse.h's; this file is the memory around it.
//
//   k_collapse LDS (static, 18 KB): sCode[1024] u32 | sPos[1024] u32 | sIdx[1024] u16 | sSeg[1025] u16 | sRank[1024] u16 | sSize[1024] u16 | sFlag[1024] u8 | part[257] u32
//   The gather reads one 4-byte code per row (codes[doc], the documents of a list are scattered: one sector each) and stores it at the row's own index, so the
//   64 lanes of a wave hit 64 consecutive banks.  The sort moves 2-byte row indices only.
#define CLP_FN __device__ __forceinline__
#include "collapse.h"
#define CLP_THREADS 256

struct DevCollapse { const uint32_t* codes; uint32_t qi, keep; };       // one collapsing query: its column's codes by document, its index in the batch, rows kept per group
struct DevCollapseIo {
    // the windows: `depth` rows per collapsing query, in list order (slot = blockIdx.x)
    const long long* wKeys; const float* wScores; const uint8_t* wTies; const int32_t* wDocs; uint32_t depth;
    // the batch buffers, `stride` rows per query
    long long* keys; float* scores; uint8_t* ties; int32_t* docs; uint32_t* counts; uint32_t stride;
    // what the step keeps per collapsing query: of each returned row its document, group code and group size (`stride` each), the groups and the rows of L, the rows written
    int32_t* rDocs; uint32_t* rCodes; uint32_t* rSizes; uint32_t* groups; uint32_t* ranked; uint32_t* returned;
};

__global__ __launch_bounds__(CLP_THREADS) void k_collapse(const DevCollapse* __restrict__ list, const infx_fused_query* __restrict__ fqs, DevCollapseIo io) {
    __shared__ uint32_t sCode[CLP_MAX_ROWS], sPos[CLP_MAX_ROWS], part[CLP_THREADS + 1];
    __shared__ uint16_t sIdx[CLP_MAX_ROWS], sSeg[CLP_MAX_ROWS + 1], sRank[CLP_MAX_ROWS], sSize[CLP_MAX_ROWS];
    __shared__ uint8_t sFlag[CLP_MAX_ROWS];
    const uint32_t slot = blockIdx.x; const int tid = threadIdx.x;
    const DevCollapse D = list[slot];
    const uint32_t n = min(min(io.counts[D.qi], io.depth), CLP_MAX_ROWS);           // rows of L (k_finalize's count)
    const uint32_t mr = (uint32_t)max(0, min(fqs[D.qi].max_results, (int)io.stride));
    const size_t w = (size_t)slot * io.depth, o = (size_t)D.qi * io.stride, r = (size_t)slot * io.stride;
    uint32_t n2 = 2; while (n2 < n) n2 <<= 1;
    for (uint32_t i = tid; i < n2; i += CLP_THREADS) { if (i < n) sCode[i] = D.codes[io.wDocs[w + i]]; sIdx[i] = (uint16_t)i; }
    __syncthreads();
    if (n > 1) wg_bitonic_idx(sIdx, n2, tid, CLP_THREADS, [&](uint16_t a, uint16_t b) { return clp_before(sCode, n, a, b); });
    for (uint32_t p = tid; p < n; p += CLP_THREADS) sFlag[p] = (uint8_t)clp_starts(sCode, sIdx, p);
    __syncthreads();
    const uint32_t groups = wg_scan_flags(sFlag, sPos, n, part, tid, CLP_THREADS);
    for (uint32_t p = tid; p < n; p += CLP_THREADS) if (sFlag[p]) sSeg[sPos[p]] = (uint16_t)p;
    if (tid == 0) sSeg[groups] = (uint16_t)n;
    __syncthreads();
    for (uint32_t p = tid; p < n; p += CLP_THREADS) {
        const uint32_t g = clp_segment(sPos[p], sFlag[p]), row = sIdx[p];
        sRank[row] = (uint16_t)clp_rank(sSeg, g, p); sSize[row] = (uint16_t)clp_size(sSeg, g);
    }
    __syncthreads();
    for (uint32_t i = tid; i < n; i += CLP_THREADS) sFlag[i] = (uint8_t)clp_keeps(sRank[i], D.keep);
    __syncthreads();
    const uint32_t kept = wg_scan_flags(sFlag, sPos, n, part, tid, CLP_THREADS);
    const uint32_t nOut = clp_returned(kept, mr);
    for (uint32_t i = tid; i < n; i += CLP_THREADS) if (clp_emits(sFlag[i], sPos[i], nOut)) {
        const uint32_t at = sPos[i];
        io.keys[o + at] = io.wKeys[w + i]; io.scores[o + at] = io.wScores[w + i]; if (io.ties) io.ties[o + at] = io.wTies[w + i];
        const int32_t d = io.wDocs[w + i];
        io.docs[o + at] = d; io.rDocs[r + at] = d; io.rCodes[r + at] = sCode[i]; io.rSizes[r + at] = sSize[i];
    }
    if (tid == 0) { io.counts[D.qi] = nOut; io.groups[slot] = groups; io.ranked[slot] = n; io.returned[slot] = nOut; }
}
