"""ctypes binding of libinfidex_hip.so with the reference's public names for the hot path.

Mirrors (reference paths under src/Infidex): SearchEngine.cs (CreateDefault/CreateMinimal/IndexDocuments/Search),
Api/Query.cs, Api/Boost.cs, Api/BoostStrength.cs, Api/Result.cs, Core/Document.cs, Api/Weight.cs, Core/ScoreEntry.cs, Coverage/CoverageSetup.cs.
"""
import ctypes as C
import os
from dataclasses import dataclass, field as _dc_field
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libinfidex_hip.so")

INFX_NFEAT = 32
STATUS = {0: "INFX_OK", 1: "INFX_EINVAL", 2: "INFX_ENOMEM", 3: "INFX_EHIP", 4: "INFX_ECAPACITY", 5: "INFX_EUNSUPPORTED"}


class InfidexError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{STATUS.get(code, code)}: {msg}")
        self.code = code


class Weight:      # Api/Weight.cs:7-26
    High, Med, Low = 0, 1, 2


@dataclass
class Field:       # Api/Field.cs (name, value, weight)
    name: str
    value: str
    weight: int = Weight.Med


@dataclass
class Document:    # Core/Document.cs:76-88 (single text => one 'content' field, Weight.Med)
    document_key: int
    fields: Union[str, Sequence[Field]]

    def field_list(self) -> List[Field]:
        return [Field("content", self.fields, Weight.Med)] if isinstance(self.fields, str) else list(self.fields)


class BoostStrength:    # Api/BoostStrength.cs
    Low, Med, High = 1, 2, 3


@dataclass
class Boost:       # Api/Boost.cs: documents matching the filter get +strength on their score (ResultProcessor.ApplyBoosts)
    filter: Optional[str]                  # Infiscript expression; None = a Boost whose Filter is null (ignored)
    strength: int = BoostStrength.Med


@dataclass
class CoverageSetup:    # Coverage/CoverageSetup.cs:6-103 (names and defaults)
    """The Stage-2 settings.  Engine-wide (SearchEngine(coverage_setup=...)) every member applies; on a Query only the six that SearchPipeline itself
    reads do — truncate, coverage_min_word_hits_abs, coverage_min_word_hits_relative, truncation_score, coverage_q_limit_for_error_tolerance,
    coverage_lcs_error_tolerance_relativeq — because the matchers keep the engine's object, as in the reference."""
    min_word_size: int = 2
    levenshtein_max_word_size: int = 20
    num_typos: int = 2                     # 0, 1 or 2 (more behaves as 2)
    min_length_one_typo: int = 3
    min_length_two_typos: int = 7
    coverage_min_word_hits_abs: int = 1
    coverage_min_word_hits_relative: int = 0
    coverage_q_limit_for_error_tolerance: int = 5
    coverage_lcs_error_tolerance_relativeq: float = 0.2
    cover_whole_query: bool = True
    cover_whole_words: bool = True
    cover_fuzzy_words: bool = True
    cover_joined_words: bool = True
    cover_prefix_suffix: bool = True
    truncate: bool = True
    enable_lexical_prescreen: bool = False     # not implemented: refused (INFX_EUNSUPPORTED)
    truncation_score: int = 254
    coverage_depth: int = 500              # never read (Query.coverage_depth is used instead): carried for shape only

    @classmethod
    def create_default(cls):
        return cls()

    @classmethod
    def create_minimal(cls):               # CoverageSetup.cs:153-162: exact matching only
        return cls(cover_whole_words=True, cover_fuzzy_words=False, cover_joined_words=False, cover_prefix_suffix=False, cover_whole_query=False)


@dataclass
class Query:       # Api/Query.cs:9-45
    text: str
    max_number_of_records_to_return: int = 10
    coverage_depth: int = 500
    enable_coverage: bool = True
    filter: Optional[str] = None           # Infiscript expression (Filter.Parse), applied to the returned rows (ResultProcessor.ApplyFilter)
    enable_facets: bool = False
    enable_boost: bool = False             # Query.EnableBoost: Boosts apply only when set
    boosts: Optional[Sequence[Boost]] = None
    sort_by: Optional[str] = None          # Query.SortBy: a field (column) name, None = relevance order
    sort_ascending: bool = False           # Query.SortAscending
    coverage_setup: Optional[CoverageSetup] = None      # Query.CoverageSetup: None = the engine's (its matcher members are ignored, see CoverageSetup)
    # Not in the reference: Result.highlights — per returned row which document word each Stage-2 query word matched and how, the spans a UI paints and a
    # snippet of at most highlight_chars (16 .. 512) UTF-16 units of the stored text (SearchEngine.stored_text), computed on the device by Stage 2's matchers.
    # Keyword-only, so they stand here without moving a positional parameter: the constructor takes them behind collapse_keep, and the dataclass's field list
    # still ends with collapse_by, collapse_keep, which callers rely on.
    highlight: bool = _dc_field(default=False, kw_only=True)
    highlight_chars: int = _dc_field(default=160, kw_only=True)
    # Not in the reference: an Infiscript expression that restricts the set that is RANKED — the query returns what it would if every document the expression
    # does not accept were deleted (index statistics untouched).  `filter` then post-processes the returned rows as usual.
    pre_filter: Optional[str] = None
    # ... and the facets of that set: Result.pre_filter_facets = the facets of every live document pre_filter accepts (SearchEngine.facets_of_documents),
    # what a drill-down sidebar shows beside the ranked rows.  Ignored without a pre_filter.
    pre_filter_facets: bool = False
    # Not in the reference: at most collapse_keep rows per value of the field collapse_by ("one hit per product family", "three results per shop").  The rows
    # kept are the first of each group in the query's whole ranked list (up to coverage_depth rows), in rank order; filter, facets, boosts and sort_by then work
    # on the returned rows.  Result.group_values / group_sizes / total_groups / total_ranked describe the fold.  None = no collapsing.
    collapse_by: Optional[str] = None
    collapse_keep: int = 1                 # rows kept per group, 1 .. 16

    @property
    def max_boost(self) -> int:           # Query.MaxBoost: the sum of every boost's strength when boosting is enabled
        if not self.enable_boost or self.boosts is None:
            return 0
        return sum(int(b.strength) for b in self.boosts)


HIGHLIGHT_KINDS = ("none", "whole", "joined_query", "joined_doc", "prefix", "suffix", "infix", "tail", "fuzzy_prefix", "fuzzy")      # HL_K_* of csrc/highlight.h
HIGHLIGHT_STATUS = ("ok", "too_long", "long_query")                                                                                  # HL_OK, HL_TOO_LONG, HL_LONG_QUERY
HIGHLIGHT_MAX_SPANS = 64


@dataclass
class TermMatch:   # Query.highlight: what one Stage-2 query word matched in one returned document (offsets and lengths: UTF-16 units of the stored text)
    word: str
    kind: str = "none"         # one of HIGHLIGHT_KINDS
    offset: int = 0            # the first occurrence of the matched document word (what Stage 2 feeds into FirstMatchIndex)
    length: int = 0
    match_offset: int = 0      # the part of that word the query word covers
    match_length: int = 0
    distance: int = 0          # edit distance of a fuzzy or fuzzy_prefix match
    offset2: int = 0           # joined_doc: the second of the two consecutive document words
    length2: int = 0


@dataclass
class Highlight:   # Query.highlight: one returned row
    status: str = "ok"         # "ok", "too_long" (the document has more than 192 Stage-2 words) or "long_query" (the query is outside the fast envelope)
    document_index: int = 0    # internal index of the document the row stands for (the segment that was scored)
    terms: List[TermMatch] = _dc_field(default_factory=list)       # one per Stage-2 query word, in Stage 2's order
    spans: List[Tuple[int, int, int, int, int]] = _dc_field(default_factory=list)      # (offset, length, match_offset, match_length, term), ascending offset, at most 64
    truncated: bool = False    # occurrences beyond the 64th were left out
    snippet: str = ""          # stored_text[snippet_start : snippet_start + n] in UTF-16 units, n <= highlight_chars
    snippet_start: int = 0
    words: int = 0             # raw words of the document under the batch's min_word_size (Stage 2's DocTokenCount)


@dataclass
class ScoreEntry:  # Core/ScoreEntry.cs
    score: float
    document_id: int
    tiebreaker: int = 0


@dataclass
class Result:      # Api/Result.cs
    records: List[ScoreEntry] = _dc_field(default_factory=list)
    unsupported: bool = False
    used_coverage: bool = False
    stage1_fallback: bool = False
    skipped_candidates: bool = False       # a candidate document exceeded the Stage-2 envelope (INFX_MAX_DOC_TOKENS) and was left out
    facets: Optional[dict] = None          # field -> [(value, count)] (count desc, value asc), Api/Result.cs Facets
    total_in_filter: int = 0               # Filter.NumberOfDocumentsInFilter
    total_in_pre_filter: int = 0           # live documents Query.pre_filter accepts (0 without one)
    error: Optional[str] = None            # search_queries: why this query alone was rejected (empty result); None when it ran

    # Query.pre_filter_facets: the facets of the documents Query.pre_filter accepts (None: not asked for, or refused).  Set by search_queries; a plain
    # attribute, not a dataclass field: the constructor's positional fields end with total_in_filter, total_in_pre_filter and error, which callers rely on.
    pre_filter_facets = None
    # Query.collapse_by (None for a query without it, or refused): per returned row the text of its group (as GroupListing.group_values spells it) and the rows
    # of the ranked list in that group, itself included ("+12 more from this shop"); the distinct groups of the ranked list; its length.  Plain attributes too.
    group_values = None
    group_sizes = None
    total_groups = None
    total_ranked = None
    # Query.highlight (None for a query without it, or refused): one Highlight per entry of `records`, as the rows finally come back.  A plain attribute too.
    highlights = None

    # SearchEngine.cs:312-316: index and score of the last returned row, and the row count
    @property
    def truncation_index(self) -> int:
        return len(self.records) - 1 if self.records else 0

    @property
    def truncation_score(self) -> float:
        return self.records[-1].score if self.records else 0.0

    @property
    def total_candidates(self) -> int:
        return len(self.records)


@dataclass
class FilteredFacets:      # SearchEngine.facets_of_documents: one per expression
    facets: dict = _dc_field(default_factory=dict)      # field -> [(value, count)] over the live documents the expression accepts (count desc, value asc, at most 100)
    total: int = 0                                      # how many live documents it accepts
    error: Optional[str] = None                         # why this expression alone was refused (syntax error, MATCHES); None when it was counted


@dataclass
class ListRequest:         # SearchEngine.list_documents: one page of one listing
    filter: Optional[str] = None        # Infiscript expression over the documents' own fields; None: every live document
    order_by: Optional[str] = None      # field whose values order the documents; None: index order
    ascending: bool = True              # False: largest value first — documents of equal value still by ascending index
    offset: int = 0                     # position of the page's first row in the whole order, 0 <= offset < 2**31
    limit: int = 20                     # rows of the page, 1 .. 1024


@dataclass
class Listing:             # SearchEngine.list_documents: one per request
    document_ids: list = _dc_field(default_factory=list)      # DocumentKeys of the page's rows, in order
    values: list = _dc_field(default_factory=list)            # the rows' order_by values as text (ToString()); [] when order_by is None
    total: int = 0                                            # live documents the filter accepts, whatever the page
    error: Optional[str] = None                               # why this request alone was refused; None when it was answered


@dataclass
class GroupListRequest:    # SearchEngine.list_groups: one page of one collapsed listing
    filter: Optional[str] = None        # Infiscript expression over the documents' own fields; None: every live document
    group_by: Optional[str] = None      # field whose values form the groups: any column, any number of distinct values (required)
    order_by: Optional[str] = None      # field whose values order the documents; None: index order
    ascending: bool = True              # False: largest value first — documents of equal value still by ascending index
    offset: int = 0                     # position of the page's first row among the groups' heads, 0 <= offset < 2**31
    limit: int = 20                     # rows of the page, 1 .. 1024


@dataclass
class GroupListing:        # SearchEngine.list_groups: one per request
    document_ids: list = _dc_field(default_factory=list)      # DocumentKeys of the page's rows: each the head of its group, the member first in the order
    values: list = _dc_field(default_factory=list)            # the rows' order_by values as text (ToString()); [] when order_by is None
    group_values: list = _dc_field(default_factory=list)      # the rows' group_by values as text (the facet key, GroupStats.value)
    group_sizes: list = _dc_field(default_factory=list)       # members of each row's group among the documents the filter accepts
    total_groups: int = 0                                     # groups with a member: the exact distinct count of group_by over the filter
    total: int = 0                                            # live documents the filter accepts (Listing.total of the same filter)
    error: Optional[str] = None                               # why this request alone was refused; None when it was answered


@dataclass
class GroupMembersRequest:  # SearchEngine.list_group_members: one page of one collapsed listing, with the first members of every group
    filter: Optional[str] = None        # Infiscript expression over the documents' own fields; None: every live document
    group_by: Optional[str] = None      # field whose values form the groups: any column, any number of distinct values (required)
    order_by: Optional[str] = None      # field whose values order the groups' heads AND the members of every group; None: index order
    ascending: bool = True              # False: largest value first — documents of equal value still by ascending index
    per_group: int = 3                  # members listed per group, 1 .. 16; limit * per_group <= 4096
    offset: int = 0                     # position of the page's first group among the groups' heads, 0 <= offset < 2**31
    limit: int = 20                     # groups of the page, 1 .. 1024


@dataclass
class GroupMembers:        # SearchEngine.list_group_members: one group of one page
    group_value: str = ""                                     # the group's value of the group_by field as text (GroupListing.group_values)
    size: int = 0                                             # members of the group among the documents the filter accepts (GroupListing.group_sizes)
    document_ids: list = _dc_field(default_factory=list)      # DocumentKeys of its first min(per_group, size) members in the listing's order, the head first
    values: list = _dc_field(default_factory=list)            # the members' order_by values as text (ToString()); [] when order_by is None


@dataclass
class GroupMembersListing:  # SearchEngine.list_group_members: one per request
    groups: list = _dc_field(default_factory=list)            # [GroupMembers] of the page: the rows of list_groups for the same request, in its order
    total_groups: int = 0                                     # groups with a member (GroupListing.total_groups)
    total: int = 0                                            # live documents the filter accepts (Listing.total of the same filter)
    error: Optional[str] = None                               # why this request alone was refused; None when it was answered


@dataclass
class TopGroupsRequest:    # SearchEngine.top_groups: one page of one ranking of a field's groups
    filter: Optional[str] = None        # Infiscript expression over the documents' own fields; None: every live document
    group_by: Optional[str] = None      # field whose values form the groups: any column, any number of distinct values (required)
    by: str = "size"                    # the figure that ranks the groups: "size", "count", "min", "max", "sum" or "mean"
    field: Optional[str] = None         # an int64 or a double column field_stats can sum; None only with by="size"
    ascending: bool = False             # False: largest figure first; groups without a figure come last and ties go by the group's value in both directions
    offset: int = 0                     # position of the page's first row in the ranking, 0 <= offset < 2**31
    limit: int = 20                     # rows of the page, 1 .. 1024


@dataclass
class GroupRow:            # SearchEngine.top_groups: one group of one page
    value: str = ""                                           # the group's value of the group_by field as text (GroupStats.value)
    size: int = 0                                             # members of the group among the documents the filter accepts
    count: Optional[int] = None                               # GroupStats' figures of the group for the request's field, from the same functions;
    nan: Optional[int] = None                                 # None without a field
    min: Optional[object] = None
    max: Optional[object] = None
    sum: Optional[object] = None
    mean: Optional[float] = None


@dataclass
class TopGroups:           # SearchEngine.top_groups: one per request
    groups: list = _dc_field(default_factory=list)            # [GroupRow] of the page, in ranking order
    total_groups: int = 0                                     # groups with a member (GroupListing.total_groups of the same filter and group_by)
    total: int = 0                                            # live documents the filter accepts (Listing.total of the same filter)
    error: Optional[str] = None                               # why this request alone was refused; None when it was answered


@dataclass
class DistinctRequest:     # SearchEngine.field_distinct: the distinct values of one field over one filter, whole and per group
    filter: Optional[str] = None        # Infiscript expression over the documents' own fields; None: every live document
    field: Optional[str] = None         # any column: int64, double or string, of any number of distinct values
    group_by: Optional[str] = None      # any column of at most 4096 distinct values; None: the whole only


@dataclass
class GroupDistinct:       # SearchEngine.field_distinct: one group of one request
    value: str = ""                                           # the group's value of the group_by field as text (GroupStats.value)
    size: int = 0                                             # members of the group among the documents the filter accepts
    distinct: int = 0                                         # distinct values of the field among them


@dataclass
class FieldDistinct:       # SearchEngine.field_distinct: one per request
    distinct: int = 0                                         # distinct values of the field among the documents the filter accepts (GroupListing.total_groups of
    #                                                           the same filter with group_by=field), with or without group_by
    total: int = 0                                            # live documents the filter accepts (Listing.total of the same filter)
    groups: list = _dc_field(default_factory=list)            # [GroupDistinct] of every group with a member, in FieldStats.groups' order; [] without group_by
    error: Optional[str] = None                               # why this request alone was refused; None when it was answered


@dataclass
class RangeRequest:        # SearchEngine.range_facets: the buckets of one numeric field over one filter
    filter: Optional[str] = None        # Infiscript expression over the documents' own fields; None: every live document
    field: str = ""                     # an int64 or a double column
    edges: tuple = ()                   # 2 .. 257 strictly increasing edges e_0 < .. < e_B: B half-open buckets [e_i, e_i+1); ints for an int column


@dataclass
class RangeFacets:         # SearchEngine.range_facets: one per request
    edges: tuple = ()                                         # the request's edges
    counts: list = _dc_field(default_factory=list)            # counts[i]: documents with edges[i] <= value < edges[i + 1]
    below: int = 0                                            # documents with value < edges[0]
    above: int = 0                                            # documents with value >= edges[-1]
    nan: int = 0                                              # documents whose value is a NaN (double columns): in no bucket, not in min / max
    total: int = 0                                            # live documents the filter accepts: nan + below + sum(counts) + above
    min: Optional[object] = None                              # smallest / largest non-NaN value of the set (int for an int column, float for a double one);
    max: Optional[object] = None                              # None when there is none
    error: Optional[str] = None                               # why this request alone was refused; None when it was answered


@dataclass
class StatsRequest:        # SearchEngine.field_stats: the statistics of one numeric field over one filter, whole or per group
    filter: Optional[str] = None        # Infiscript expression over the documents' own fields; None: every live document
    field: Optional[str] = None         # an int64 or a double column
    group_by: Optional[str] = None      # any column of at most 4096 distinct values; None: the whole only


@dataclass
class GroupStats:          # SearchEngine.field_stats: one group of one request
    value: str = ""                                           # the group's value of the group_by field as text (ToString(), the facet key)
    count: int = 0                                            # members whose value is not a NaN
    nan: int = 0                                              # members whose value is a NaN: in no other figure
    min: Optional[object] = None                              # smallest / largest non-NaN value (int for an int column, float for a double one); None when
    max: Optional[object] = None                              # count == 0
    sum: object = 0                                           # int column: the exact sum, a Python int; double column: the exact real sum rounded once
    mean: Optional[float] = None                              # the exact sum / count rounded once; None when count == 0


@dataclass
class FieldStats:          # SearchEngine.field_stats: one per request
    count: int = 0                                            # members whose value is not a NaN
    nan: int = 0                                              # members whose value is a NaN (double columns): in no other figure
    total: int = 0                                            # live documents the filter accepts: count + nan (Listing.total of the same filter)
    min: Optional[object] = None                              # smallest / largest non-NaN value of the set, as RangeFacets.min / max; None when count == 0
    max: Optional[object] = None
    sum: object = 0                                           # int column: the exact sum, a Python int (it may exceed 64 bits); double column: the exact real sum
    #                                                           of the finite values rounded once (math.fsum's), +-inf / NaN with infinite members
    mean: Optional[float] = None                              # the exact sum / count rounded once; None when count == 0
    groups: list = _dc_field(default_factory=list)            # [GroupStats] of every group with a member: members descending, then value ascending; [] without group_by
    error: Optional[str] = None                               # why this request alone was refused; None when it was answered


@dataclass
class BucketStatsRequest:  # SearchEngine.bucket_stats: the statistics of one numeric field per range bucket of a second one, over one filter
    filter: Optional[str] = None        # Infiscript expression over the documents' own fields; None: every live document
    field: Optional[str] = None         # the summed field: an int64 or a double column field_stats can sum
    bucket_by: Optional[str] = None     # the field the buckets cut: an int64 or a double column; it may be `field`
    edges: tuple = ()                   # 2 .. 257 strictly increasing edges e_0 < .. < e_B over bucket_by, as RangeRequest.edges


@dataclass
class BucketRow:           # SearchEngine.bucket_stats: one bucket (or below / above / nan, or the whole) of one request
    size: int = 0                                             # members of the row: count + nan
    count: int = 0                                            # members whose value of `field` is not a NaN
    nan: int = 0                                              # members whose value of `field` is a NaN: in no other figure
    min: Optional[object] = None                              # smallest / largest non-NaN value of `field` (int for an int column, float for a double one); None
    max: Optional[object] = None                              # when count == 0
    sum: object = 0                                           # int column: the exact sum, a Python int; double column: the exact real sum rounded once
    mean: Optional[float] = None                              # the exact sum / count rounded once; None when count == 0


@dataclass
class BucketStats:         # SearchEngine.bucket_stats: one per request
    edges: tuple = ()                                         # the request's edges
    buckets: list = _dc_field(default_factory=list)           # [BucketRow]: buckets[i] the members with edges[i] <= bucket_by < edges[i + 1]
    below: BucketRow = _dc_field(default_factory=BucketRow)   # the members with bucket_by < edges[0]
    above: BucketRow = _dc_field(default_factory=BucketRow)   # the members with bucket_by >= edges[-1]
    nan: BucketRow = _dc_field(default_factory=BucketRow)     # the members whose bucket_by value is a NaN (double columns): in no bucket
    whole: BucketRow = _dc_field(default_factory=BucketRow)   # the whole set: field_stats(filter, field)'s figures
    total: int = 0                                            # live documents the filter accepts: nan.size + below.size + the buckets' sizes + above.size
    error: Optional[str] = None                               # why this request alone was refused; None when it was answered


@dataclass
class QuantileRequest:     # SearchEngine.field_quantiles: the quantiles of one numeric field over one filter, whole and per group
    filter: Optional[str] = None        # Infiscript expression over the documents' own fields; None: every live document
    field: Optional[str] = None         # an int64 or a double column
    q: tuple = (0.5,)                   # 1 .. 16 numbers in [0, 1], in any order, duplicates allowed
    group_by: Optional[str] = None      # any column of at most 4096 distinct values; None: the whole only


@dataclass
class GroupQuantiles:      # SearchEngine.field_quantiles: one group of one request
    value: str = ""                                           # the group's value of the group_by field as text (GroupStats.value)
    count: int = 0                                            # members whose value is not a NaN
    nan: int = 0                                              # members whose value is a NaN: in no quantile
    values: list = _dc_field(default_factory=list)            # values[i]: the group's value at position floor((count - 1) * q[i]); None when count == 0


@dataclass
class FieldQuantiles:      # SearchEngine.field_quantiles: one per request
    q: tuple = ()                                             # the request's quantiles, as floats
    values: list = _dc_field(default_factory=list)            # values[i]: the value at 0-based position floor((count - 1) * q[i]) of the non-NaN members in
    #                                                           ascending order (int for an int column, float for a double one); None when count == 0
    count: int = 0                                            # members whose value is not a NaN
    nan: int = 0                                              # members whose value is a NaN (double columns): in no quantile
    total: int = 0                                            # live documents the filter accepts: count + nan (Listing.total, FieldStats.total)
    groups: list = _dc_field(default_factory=list)            # [GroupQuantiles] of every group with a member, in FieldStats.groups' order; [] without group_by
    error: Optional[str] = None                               # why this request alone was refused; None when it was answered


class _QuantReq(C.Structure):          # infx_quantile_request (include/infidex_engine.h)
    _fields_ = [("filter", C.c_char_p), ("field", C.c_char_p), ("group_by", C.c_char_p), ("q", C.POINTER(C.c_double)), ("nq", C.c_uint32)]


class _QuantFigures(C.Structure):      # infx_quantile_figures (include/infidex_engine.h)
    _fields_ = [("count", C.c_uint32), ("nan", C.c_uint32), ("kind", C.c_int32), ("nq", C.c_uint32), ("v_i", C.c_int64 * 16), ("v_d", C.c_double * 16)]


class _StatsReq(C.Structure):          # infx_stats_request (include/infidex_engine.h)
    _fields_ = [("filter", C.c_char_p), ("field", C.c_char_p), ("group_by", C.c_char_p)]


class _StatsFigures(C.Structure):      # infx_stats_figures (include/infidex_engine.h)
    _fields_ = [("count", C.c_uint32), ("nan", C.c_uint32), ("kind", C.c_int32), ("reserved", C.c_int32), ("min_i", C.c_int64), ("max_i", C.c_int64),
                ("min_d", C.c_double), ("max_d", C.c_double), ("sum_d", C.c_double), ("sum_lo", C.c_uint64), ("sum_hi", C.c_int64), ("mean", C.c_double)]


class _BucketStatsReq(C.Structure):    # infx_bucket_stats_request (include/infidex_engine.h)
    _fields_ = [("filter", C.c_char_p), ("field", C.c_char_p), ("bucket_by", C.c_char_p), ("nedges", C.c_uint32), ("edges_i", C.POINTER(C.c_int64)),
                ("edges_d", C.POINTER(C.c_double))]


class _RangeReq(C.Structure):
    _fields_ = [("filter", C.c_char_p), ("field", C.c_char_p), ("nedges", C.c_uint32), ("edges_i", C.POINTER(C.c_int64)), ("edges_d", C.POINTER(C.c_double))]


class _ListReq(C.Structure):
    _fields_ = [("filter", C.c_char_p), ("order_by", C.c_char_p), ("ascending", C.c_int32), ("offset", C.c_uint32), ("limit", C.c_uint32)]


class _GroupListReq(C.Structure):     # infx_group_list_request (include/infidex_engine.h)
    _fields_ = [("filter", C.c_char_p), ("group_by", C.c_char_p), ("order_by", C.c_char_p), ("ascending", C.c_int32), ("offset", C.c_uint32), ("limit", C.c_uint32)]


class _GroupMembersReq(C.Structure):  # infx_group_members_request (include/infidex_engine.h)
    _fields_ = [("filter", C.c_char_p), ("group_by", C.c_char_p), ("order_by", C.c_char_p), ("ascending", C.c_int32), ("offset", C.c_uint32), ("limit", C.c_uint32),
                ("per_group", C.c_uint32)]


class _TopReq(C.Structure):           # infx_top_request (include/infidex_engine.h)
    _fields_ = [("filter", C.c_char_p), ("group_by", C.c_char_p), ("by", C.c_char_p), ("field", C.c_char_p), ("ascending", C.c_int32), ("offset", C.c_uint32), ("limit", C.c_uint32)]


class _DistinctReq(C.Structure):       # infx_distinct_request (include/infidex_engine.h)
    _fields_ = [("filter", C.c_char_p), ("field", C.c_char_p), ("group_by", C.c_char_p)]


class _DistinctFigures(C.Structure):   # infx_distinct_figures (include/infidex_engine.h)
    _fields_ = [("size", C.c_uint32), ("distinct", C.c_uint32)]


class _Cfg(C.Structure):
    _fields_ = [("device", C.c_int32), ("range_docs", C.c_int32), ("max_depth", C.c_int32), ("threads", C.c_int32),
                ("enable_coverage", C.c_int32), ("word_matcher", C.c_int32), ("stop_term_limit", C.c_int32),
                ("want_features", C.c_int32), ("no_exact_replay", C.c_int32)]


class _CoverageSetup(C.Structure):     # infx_coverage_setup (include/infidex_engine.h)
    _fields_ = [("min_word_size", C.c_int32), ("levenshtein_max_word_size", C.c_int32), ("num_typos", C.c_int32), ("min_length_one_typo", C.c_int32),
                ("min_length_two_typos", C.c_int32), ("coverage_min_word_hits_abs", C.c_int32), ("coverage_min_word_hits_relative", C.c_int32),
                ("coverage_q_limit_for_error_tolerance", C.c_int32), ("coverage_lcs_error_tolerance_relativeq", C.c_double),
                ("cover_whole_query", C.c_int32), ("cover_whole_words", C.c_int32), ("cover_fuzzy_words", C.c_int32), ("cover_joined_words", C.c_int32),
                ("cover_prefix_suffix", C.c_int32), ("truncate", C.c_int32), ("enable_lexical_prescreen", C.c_int32), ("truncation_score", C.c_int32)]


def _coverage_struct(cs: CoverageSetup) -> _CoverageSetup:
    st = _CoverageSetup()
    for name, ty in _CoverageSetup._fields_:
        v = getattr(cs, name)
        if ty is C.c_double:
            setattr(st, name, float(v))
        else:
            v = int(v)
            setattr(st, name, v if -2 ** 31 <= v < 2 ** 31 else -1)      # (out of the int32 range: out of the accepted range too)
    return st


_lib = None


def load_library():
    """Loads the in-tree HIP extension; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        path = os.environ.get("INFX_LIB") or LIB_PATH       # INFX_LIB: the experiments build of the same library (A/B test of the k_accumulate designs)
        if not os.path.exists(path):
            raise InfidexError(3, f"{path} not built — run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(path)
        L.infx_engine_last_error.restype = C.c_char_p
        L.infx_last_error.restype = C.c_char_p
        L.infx_engine_wordmatcher.restype = C.c_int64
        L.infx_engine_last_stage2.restype = C.c_int64
        _lib = L
    return _lib


def _u16(s: str) -> np.ndarray:
    return np.frombuffer(s.encode("utf-16-le", "surrogatepass"), dtype=np.uint16).copy()


def _p(a, ty):
    return a.ctypes.data_as(C.POINTER(ty)) if a is not None else None


def pack_texts(texts: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    arrs = [_u16(t) for t in texts]
    offs = np.zeros(len(arrs) + 1, np.uint64)
    if arrs:
        offs[1:] = np.cumsum([len(a) for a in arrs])
    arena = np.concatenate(arrs) if arrs and offs[-1] > 0 else np.zeros(1, np.uint16)
    return arena, offs


class SearchEngine:
    def __init__(self, enable_coverage=True, word_matcher=True, device: int = 0, range_docs: int = 0, max_depth: int = 500,
                 threads: int = 0, stop_term_limit: int = 0, want_features: bool = False, exact_replay: bool = True,
                 coverage_setup: Optional[CoverageSetup] = None, max_post_rows: int = 64):
        """max_post_rows (64..1024): how many returned rows per query Filter, EnableFacets, Boosts, SortBy and browse queries accept.  The reference
        post-filters the truncated top-MaxNumberOfRecordsToReturn rows, so a selective filter wants a few hundred rows to filter; the default keeps the
        64-row envelope and its refusals."""
        self.L = load_library()
        cfg = _Cfg(device, range_docs, max_depth, threads, int(enable_coverage), int(word_matcher), stop_term_limit, int(want_features), int(not exact_replay))
        h = C.c_void_p()
        self._check(self.L.infx_engine_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.device = device
        try:
            if coverage_setup is not None:
                self.set_coverage_setup(coverage_setup)
            if not 64 <= int(max_post_rows) <= 1024:          # (checked here too: ctypes would wrap a value beyond int32)
                raise InfidexError(1, "max_post_rows lies outside [64, 1024]")
            self._check(self.L.infx_engine_set_post_rows(self.h, int(max_post_rows)))
        except Exception:
            self.close()
            raise

    @property
    def max_post_rows(self) -> int:
        v = C.c_int32(0)
        self._check(self.L.infx_engine_get_post_rows(self.h, C.byref(v)))
        return int(v.value)

    def set_coverage_setup(self, coverage_setup: Optional[CoverageSetup]):
        """The engine-wide CoverageSetup (SearchEngine's coverageSetup: argument; None = the defaults).  Legal between batches."""
        st = _coverage_struct(coverage_setup) if coverage_setup is not None else None
        self._check(self.L.infx_engine_set_coverage_setup(self.h, C.byref(st) if st is not None else None))

    def coverage_setup(self) -> CoverageSetup:
        st = _CoverageSetup()
        self._check(self.L.infx_engine_get_coverage_setup(self.h, C.byref(st)))
        kw = {}
        for name, ty in _CoverageSetup._fields_:
            d = CoverageSetup.__dataclass_fields__[name].default
            kw[name] = type(d)(getattr(st, name))
        return CoverageSetup(**kw)

    # SearchEngine.cs:78-94
    @classmethod
    def create_default(cls, **kw):
        return cls(enable_coverage=True, word_matcher=True, **kw)

    @classmethod
    def create_minimal(cls, **kw):
        return cls(enable_coverage=False, word_matcher=False, **kw)

    def _check(self, rc):
        if rc != 0:
            msg = self.L.infx_engine_last_error()
            raise InfidexError(rc, msg.decode("utf-8", "replace") if msg else "")

    def close(self):
        if getattr(self, "h", None):
            self.L.infx_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- indexing ----
    def index_documents(self, docs: Sequence[Document]):
        docs = list(docs)
        if not docs:
            return self.index_flat(None, np.zeros(1, np.uint16), np.zeros(1, np.uint64), (Weight.Med,))
        fl0 = docs[0].field_list()
        weights = [f.weight for f in fl0]
        texts = []
        for d in docs:
            fl = d.field_list()
            if [f.weight for f in fl] != weights:
                raise InfidexError(1, "all documents of one IndexDocuments call must share the field schema")
            texts.extend(str(f.value) for f in fl)
        arena, offs = pack_texts(texts)
        keys = np.asarray([d.document_key for d in docs], np.int64)
        return self.index_flat(keys, arena, offs, weights)

    def index_flat(self, keys, arena, offs, field_weights=(Weight.Med,)):
        fw = np.asarray(field_weights, np.int32)
        n = (len(offs) - 1) // len(fw)
        keys = None if keys is None else np.ascontiguousarray(keys, np.int64)
        self._keep = (keys, arena, offs)
        self._check(self.L.infx_engine_index_documents(self.h, C.c_int64(n), _p(keys, C.c_int64), _p(arena, C.c_uint16),
                                                       _p(offs, C.c_uint64), len(fw), _p(fw, C.c_int32)))
        self._keep = None

    def index_flat_from_segments(self, keys, arena, offs, field_weights, segment_paths, doc_bases):
        """An engine populated from flushed INFS segments + a live tail (VectorModel.Flush): the posting lists of the flushed document ranges come from the
        files, the documents supply everything else (infx_engine_index_from_segments); the corpus is then searched as one index."""
        fw = np.asarray(field_weights, np.int32)
        n = (len(offs) - 1) // len(fw)
        keys = None if keys is None else np.ascontiguousarray(keys, np.int64)
        paths = (C.c_char_p * len(segment_paths))(*[str(p).encode() for p in segment_paths])
        bases = np.ascontiguousarray(doc_bases, np.int32)
        self._check(self.L.infx_engine_index_from_segments(self.h, C.c_int64(n), _p(keys, C.c_int64), _p(arena, C.c_uint16), _p(offs, C.c_uint64), len(fw), _p(fw, C.c_int32),
                                                            len(segment_paths), paths, _p(bases, C.c_int32)))

    def load_index(self, path: str):
        """SearchEngine.Load (SearchEngine.cs:399-441) of an INFDX2 file: indexes the stored documents and verifies every stored term / posting against
        the index just built (infx_engine_load_index).  Returns (documents, stored terms compared, stored postings compared)."""
        c = np.zeros(3, np.int64)
        self._check(self.L.infx_engine_load_index(self.h, str(path).encode(), _p(c, C.c_int64)))
        return int(c[0]), int(c[1]), int(c[2])

    # ---- one host-index build per node (document shards; include/infidex_engine.h) ----
    def set_build_threads(self, threads: int):
        """Threads of the index build only (a node's leader rank builds with every core while planning keeps the rank's share)."""
        self._check(self.L.infx_engine_set_build_threads(self.h, int(threads)))

    def save_host_index(self, path: str):
        """Writes the host index (dictionaries, postings, WordMatcher lists, texts) to a node-local file for the node's other ranks."""
        self._check(self.L.infx_engine_save_host_index(self.h, str(path).encode()))

    def index_from_host_cache(self, path: str):
        """Instead of index_flat / index_documents: reads the host index a leader rank saved and uploads this rank's shard."""
        self._check(self.L.infx_engine_index_from_host_cache(self.h, str(path).encode()))

    # ---- Document.Deleted (DocumentCollection.DeleteDocumentsByKey, Core/DocumentCollection.cs:200-212) ----
    def delete_documents(self, keys) -> int:
        """Marks every document with one of these DocumentKeys as deleted (index statistics are not rebuilt, as in the reference until the next
        re-index); returns how many documents were newly marked.  Exclusive: no search may be in flight."""
        k = np.ascontiguousarray(list(keys) if not isinstance(keys, np.ndarray) else keys, np.int64)
        marked = C.c_int64(0)
        self._check(self.L.infx_engine_delete_documents(self.h, _p(k, C.c_int64), C.c_int64(len(k)), C.byref(marked)))
        return int(marked.value)

    def delete_document_ids(self, ids) -> int:
        """Document.Deleted = true on single documents by internal id (indexing order), e.g. one of several documents of a key; returns how many were
        newly marked.  Exclusive: no search may be in flight."""
        k = np.ascontiguousarray(list(ids) if not isinstance(ids, np.ndarray) else ids, np.int64)
        marked = C.c_int64(0)
        self._check(self.L.infx_engine_delete_document_ids(self.h, _p(k, C.c_int64), C.c_int64(len(k)), C.byref(marked)))
        return int(marked.value)

    def shard_info(self):
        """(first internal id, number of documents) of the doc range this engine's GPU holds (the whole corpus when unsharded)."""
        b = C.c_int32(0); n = C.c_int32(0)
        self._check(self.L.infx_engine_shard_info(self.h, C.byref(b), C.byref(n)))
        return int(b.value), int(n.value)

    def restore_documents(self):
        """Clears every Deleted flag."""
        self._check(self.L.infx_engine_restore_documents(self.h))

    # ---- non-indexed document fields (DocumentFields) as columns: filterable / facetable (config 5) ----
    def set_column(self, name, values, facetable=False):
        """One value per indexed document, in indexing order: int64 / float64 numpy array or a sequence of str."""
        n = len(values)
        if isinstance(values, np.ndarray) and values.dtype.kind in "iu":
            v = np.ascontiguousarray(values, np.int64)
            self._check(self.L.infx_engine_add_column(self.h, name.encode(), 1, int(facetable), C.c_int64(n), _p(v, C.c_int64), None, None, None))
        elif isinstance(values, np.ndarray) and values.dtype.kind == "f":
            v = np.ascontiguousarray(values, np.float64)
            self._check(self.L.infx_engine_add_column(self.h, name.encode(), 2, int(facetable), C.c_int64(n), None, _p(v, C.c_double), None, None))
        else:
            bs = [str(x).encode() for x in values]
            offs = np.zeros(n + 1, np.uint64); offs[1:] = np.cumsum([len(b) for b in bs])
            arena = b"".join(bs) + b"\0"
            self._check(self.L.infx_engine_add_column(self.h, name.encode(), 3, int(facetable), C.c_int64(n), None, None, C.c_char_p(arena), _p(offs, C.c_uint64)))

    def set_list_column(self, name, lists, facetable=False):
        """A field that holds a LIST of values per document (a film's genres, a product's tags): one sequence per indexed document, in indexing order, possibly
        empty; all elements of a column are int, or all float, or all str.  Lists are kept as given (order and duplicates).  A filter leaf over the field
        holds for a document when it holds for at least one element — for an empty list, when it holds for a null value: `tags IS NULL` (and `<`, `<=`: a null is below every constant) accepts the
        empty lists, and `NOT tags = 'sale'` / `tags != 'sale'` mean "no element equals sale".  A facetable list column appears in facets_of_all_documents
        and facets_of_documents (and Query.pre_filter_facets), a value's count being the number of its element occurrences; not in Result.facets.  Shares
        one namespace with set_column: the newer column of a name replaces the older, of either kind.  At most 8 list columns, 4 of them facetable."""
        n = int(self.index_stats()["docs"]) if self.h else 0
        lists = [list(x) for x in lists]
        if len(lists) != n:
            raise InfidexError(1, "a list column needs one list per indexed document")
        flat = [x for l in lists for x in l]
        kinds = {1 if isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_)) else 2 if isinstance(x, (float, np.floating)) else 3 if isinstance(x, str) else 0 for x in flat}
        if len(kinds) > 1 or 0 in kinds:
            raise InfidexError(1, "the elements of a list column are all int, or all float, or all str")
        kind = kinds.pop() if kinds else 3
        doc_offs = np.zeros(n + 1, np.uint64); doc_offs[1:] = np.cumsum([len(l) for l in lists], dtype=np.uint64)
        vi = vd = arena = offs = None
        if kind == 1:
            vi = np.ascontiguousarray(flat, np.int64) if flat else np.zeros(1, np.int64)
        elif kind == 2:
            vd = np.ascontiguousarray(flat, np.float64)
        else:
            bs = [x.encode() for x in flat]
            offs = np.zeros(len(bs) + 1, np.uint64); offs[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
            arena = b"".join(bs) + b"\0"
        self._check(self.L.infx_engine_add_list_column(self.h, name.encode(), kind, int(facetable), C.c_int64(n), _p(doc_offs, C.c_uint64),
                                                       _p(vi, C.c_int64) if vi is not None else None, _p(vd, C.c_double) if vd is not None else None,
                                                       C.c_char_p(arena) if arena is not None else None, _p(offs, C.c_uint64) if offs is not None else None))

    def list_column(self, name, document_index: int) -> list:
        """The stored list of one document (internal index) in list column `name`, as it was given: ints, floats or strs."""
        lcol, kind = _list_column_index(self, name)
        if lcol < 0:
            raise InfidexError(1, "no list column named %r" % (name,))
        fn = self.L.infx_engine_list_column_document; fn.restype = C.c_int64
        m = fn(self.h, lcol, C.c_int64(int(document_index)), None, C.c_int64(0))
        if m < 0:
            self._check(1)
        codes = np.zeros(max(int(m), 1), np.uint32)
        if fn(self.h, lcol, C.c_int64(int(document_index)), _p(codes, C.c_uint32), C.c_int64(int(m))) != m:
            self._check(1)
        conv = int if kind == 1 else float if kind == 2 else str
        return [conv(_list_column_value(self, lcol, int(c))) for c in codes[:m]]

    def last_list_leaf_stats(self):
        """(derived leaf columns built, k_list_leaf launches) of the last expression the engine compiled: the list-column leaves of one expression that the
        engine had not cached are lowered in one launch per list column.  An expression taken from the filter cache compiles nothing and leaves the figures
        as they are: list_leaf_totals() shows that nothing was built."""
        b = C.c_uint32(0); l = C.c_uint32(0)
        self._check(self.L.infx_engine_last_list_leaf_stats(self.h, C.byref(b), C.byref(l)))
        return int(b.value), int(l.value)

    def list_leaf_totals(self):
        """(derived leaf columns built, k_list_leaf launches) summed over every filter the engine has compiled: a call that leaves both as they were
        launched nothing for list-column leaves."""
        b = C.c_uint64(0); l = C.c_uint64(0)
        self._check(self.L.infx_engine_list_leaf_totals(self.h, C.byref(b), C.byref(l)))
        return int(b.value), int(l.value)

    def facets_of(self, sh, nq, i):
        """Facets of query i of the last batch (nq queries) searched on session handle sh with Query.EnableFacets: {field: [(value, count)]}, counts over
        the returned rows, (count desc, value asc) — Core/FacetBuilder.cs:19-105."""
        return _facet_columns(self, self.L.infx_engine_facet_column_count(sh), lambda k, *out: self.L.infx_engine_last_facets(sh, nq, i, k, *out))

    def facets_of_all_documents(self, session=None):
        """FacetBuilder.BuildFacetsFromAllDocuments (Core/FacetBuilder.cs:110-181): {field: [(value, count)]} over every document that is not Deleted
        (per document, not per key), for every facetable column, counted in one device pass; (count desc, value asc), at most 100 values per field,
        null / empty values left out, fields without a value absent."""
        return _facets_all(self, session.h if session is not None else self._default_session())

    def facets_of_documents(self, filters, session=None):
        """The facets of the documents an Infiscript expression accepts: {field: [(value, count)]} over every document that is not Deleted and whose own
        fields the expression accepts (per document, as total_in_pre_filter counts), ordered and cut as facets_of_all_documents, plus their number.
        filters: one expression -> one FilteredFacets; a sequence -> a list, one per expression.  All expressions the engine has no cached answer for
        are evaluated and counted in one pass over the columns (16 per pass); an expression with a syntax error or MATCHES gets `error` set, alone."""
        return _facets_filtered(self, session.h if session is not None else self._default_session(), filters)

    def last_filtered_facet_stats(self, session=None):
        """(expressions counted on the device, expressions taken from the engine's cache, k_facets_filtered launches) of the session's last
        facets_of_documents call (or batch with Query.pre_filter_facets)."""
        return _u32_stats(self, "infx_engine_last_facets_filtered_stats", session.h if session is not None else self._default_session(), 3)

    def list_documents(self, filter=None, order_by=None, ascending=True, offset=0, limit=20, session=None):
        """A page of the documents a filter accepts, in the order of a field (not in the reference).  The set: every document that is not Deleted and whose
        own fields `filter` accepts (None: every live document; exactly the documents total_in_pre_filter counts; duplicate keys are rows of their own).
        The order: order_by's values as Query.sort_by compares them (None: index order), descending when ascending is False, documents of equal value by
        ascending internal index in both directions — a total order, so consecutive pages never overlap or skip.  Returns Listing(document_ids, values,
        total, error) for positions [offset, offset + limit), 1 <= limit <= 1024 whatever max_post_rows is; an offset at or beyond the total gives an
        empty page.  The device selects the page (a radix select over the sort ranks of the set, no sort of the set; a deep offset costs what offset 0
        costs) and the session's pre-filter masks are reused across pages.  A sequence of ListRequest as first argument -> a list of Listing, sixteen
        requests per device call; a request with a syntax error, MATCHES, an unknown field or a limit out of range gets `error` set, alone."""
        return _list_documents(self, session.h if session is not None else self._default_session(), filter, order_by, ascending, offset, limit)

    def last_list_stats(self, session=None):
        """(masks built, masks reused, histogram passes, kernel launches) of the session's last list_documents device call."""
        return _u32_stats(self, "infx_engine_last_list_stats", session.h if session is not None else self._default_session(), 4)

    def set_list_digit_bits(self, bits, session=None):
        """The width of a radix-select digit of list_documents on the session, 4 .. 11 (default 11): a tuning knob, the pages do not depend on it."""
        self._check(self.L.infx_engine_set_list_digit_bits(session.h if session is not None else self._default_session(), int(bits)))

    def list_groups(self, filter=None, group_by=None, order_by=None, ascending=True, offset=0, limit=20, session=None):
        """A collapsed listing (not in the reference): over the documents list_documents(filter) lists and in its order (order_by, ascending; ties by ascending
        internal index in both directions), one row per value of `group_by` — the group's head, its member that comes first in that order ("the cheapest
        offer of every product", "the newest post of every author") — and of those rows the page [offset, offset + limit).  A group is one dictionary code
        of group_by, exactly as field_stats(group_by=...) forms and names groups; any column of any kind and any number of values, group_by == order_by
        included.  The answer equals list_documents over the filter's documents restricted to the heads, so pages never overlap or skip.  Returns
        GroupListing(document_ids, values, group_values, group_sizes, total_groups, total, error): group_sizes the members of each row's group, total_groups
        the exact distinct count of group_by over the filter, total = Listing.total.  1 <= limit <= 1024; offset >= total_groups is an empty page.  A
        sequence of GroupListRequest as first argument -> a list of GroupListing, sixteen requests per device call; the pages of one listing in one call
        share one pass over the corpus.  Exact and deterministic; nothing is cached but the session's pre-filter masks.  Needs a GPU."""
        return _list_groups(self, session.h if session is not None else self._default_session(), filter, group_by, order_by, ascending, offset, limit)

    def last_group_list_stats(self, session=None):
        """(masks built, masks reused, head passes, histogram passes, kernel launches) of the session's last list_groups device call."""
        return _u32_stats(self, "infx_engine_last_group_list_stats", session.h if session is not None else self._default_session(), 5)

    def list_group_members(self, filter=None, group_by=None, order_by=None, ascending=True, per_group=3, offset=0, limit=20, session=None):
        """The first members of every group, by page (not in the reference): the groups are exactly the rows of list_groups(filter, group_by, order_by,
        ascending, offset, limit), in its order — by each group's head — and every group carries its first min(per_group, size) members in
        list_documents(filter, order_by, ascending)'s order (ties by ascending internal index in both directions; duplicate DocumentKeys are members of their
        own): "the three cheapest offers of every product family, page 7".  Returns GroupMembersListing(groups, total_groups, total, error), groups the
        GroupMembers(group_value, size, document_ids, values) of the page: document_ids[0] is list_groups' head, size, total_groups and total are
        list_groups'; values is [] without order_by.  1 <= per_group <= 16, 1 <= limit <= 1024, limit * per_group <= 4096; offset >= total_groups is an
        empty page.  A sequence of GroupMembersRequest as first argument -> a list of GroupMembersListing, sixteen requests per device call.  One call
        in place of one list_documents per row: the members are kept in the walk that counts the sizes (profiles/group_members.md).  Exact and deterministic; nothing is cached but the session's
        pre-filter masks.  Needs a GPU."""
        return _list_group_members(self, session.h if session is not None else self._default_session(), filter, group_by, order_by, ascending, per_group, offset, limit)

    def last_group_members_stats(self, session=None):
        """(masks built, masks reused, head passes, histogram passes, member walks, kernel launches) of the session's last list_group_members device call."""
        return _u32_stats(self, "infx_engine_last_group_members_stats", session.h if session is not None else self._default_session(), 6)

    def top_groups(self, filter=None, group_by=None, by="size", field=None, ascending=False, offset=0, limit=20, session=None):
        """A field's groups ranked by a figure and cut to a page (not in the reference): over the documents list_documents(filter) lists, one row per value
        of group_by (any column, any number of distinct values — field_stats stops at 4096 — a unique column and `field` itself included) that has a member,
        ranked by `by`: "size" the group's members, or for `field` (an int64 or double column field_stats can sum) "count", "min", "max", "sum" or "mean" —
        GroupStats' figures, compared as the caller sees them (an int sum exactly, min / max as Query.sort_by compares values).  Groups without a figure (min /
        max / mean with count == 0, a sum or mean over both infinities) come after all others in BOTH directions; every tie goes by the group's value
        ascending (field_stats' order of equal groups) in both directions, so pages never overlap or skip.  1 <= limit <= 1024, 0 <= offset < 2**31.  Returns
        TopGroups(groups, total_groups, total, error): groups the GroupRow(value, size, count, nan, min, max, sum, mean) of rows [offset, offset + limit) —
        the six figures exactly what field_stats returns for that group, None without a field.  A sequence of TopGroupsRequest as first argument -> a list of
        TopGroups, sixteen requests per device call; pages, directions and `by`s of one (filter, field, group_by) in one call share one pass over the
        documents.  A refused request gets `error` set, alone.  Exact and deterministic; needs a GPU."""
        return _top_groups(self, session.h if session is not None else self._default_session(), filter, group_by, by, field, ascending, offset, limit)

    def last_top_groups_stats(self, session=None):
        """(masks built, masks reused, accumulate passes, select passes, kernel launches) of the session's last top_groups device call."""
        return _u32_stats(self, "infx_engine_last_top_groups_stats", session.h if session is not None else self._default_session(), 5)

    def last_top_groups_placement(self, session=None):
        """(tables accumulated in a workgroup's LDS, in a CU's whole LDS, in global memory) of the session's last top_groups device call."""
        return _u32_stats(self, "infx_engine_last_top_groups_placement", session.h if session is not None else self._default_session(), 3)

    def field_distinct(self, filter=None, field=None, group_by=None, session=None):
        """Exact distinct counts (not in the reference): over the documents list_documents(filter) lists, the number of distinct values of `field` — any
        column of any kind and any number of values, a string column and a unique column included — whole and, with group_by (any column of at most 4096
        values, checked as field_stats checks it; it may be `field` itself), per group.  A value is one dictionary code of the field, exactly the groups
        list_groups(group_by=field) forms: `distinct` equals that call's total_groups.  Values are told apart by their stored bytes: a double by its bit
        pattern, so -0.0 and 0.0 are two values, a NaN is a value and NaNs of different payloads differ.  Returns FieldDistinct(distinct, total, groups,
        error): groups the GroupDistinct(value, size, distinct) of every group with a member in FieldStats.groups' order, [] without group_by; the whole
        set's distinct is filled either way.  A sequence of DistinctRequest as first argument -> a list of FieldDistinct, sixteen requests per device call;
        requests that share filter, field and group_by share one pass.  A refused request gets `error` set, alone.  Exact and deterministic — no sketch;
        needs a GPU."""
        return _field_distinct(self, session.h if session is not None else self._default_session(), filter, field, group_by)

    def last_field_distinct_stats(self, session=None):
        """(masks built, masks reused, passes that marked in LDS, in a global bitmap, in a hash set, kernel launches) of the session's last field_distinct
        device call."""
        return _u32_stats(self, "infx_engine_last_field_distinct_stats", session.h if session is not None else self._default_session(), 6)

    def set_distinct_placement(self, mode, session=None):
        """Where field_distinct marks on this session: 0 automatic (default), 1 LDS, 2 global bitmap, 3 hash set; a forced placement that does not fit falls
        to the next larger one.  The answers do not depend on it — for tests and measurements."""
        self._check(self.L.infx_engine_set_distinct_placement(session.h if session is not None else self._default_session(), int(mode)))

    def range_facets(self, filter=None, field=None, edges=(), session=None):
        """Range facets (not in the reference): over the documents list_documents(filter) lists — not Deleted, their own fields accepted by `filter`; None:
        every live document; duplicate keys are documents of their own — the values of `field`, an int64 or a double column, counted into the half-open
        buckets [edges[i], edges[i + 1]) (the last one too), with the documents below edges[0], at or above edges[-1] and, on a double column, with a NaN
        value (in no bucket), the size of the set and its smallest and largest non-NaN value.  Returns RangeFacets(edges, counts, below, above, nan, total,
        min, max, error); always nan + below + sum(counts) + above == total.  2 .. 257 edges, strictly increasing as Query.sort_by compares values (-0.0,
        0.0 is not), no NaN, +-inf allowed on a double column; an int column takes Python ints.  A sequence of RangeRequest as first argument -> a list of
        RangeFacets, sixteen requests per device call, all counted in ONE pass over the corpus (requests of one filter read its mask once); a request
        with a syntax error, MATCHES, an unknown or string field or bad edges gets `error` set, alone.  No sums or means (per bucket: bucket_stats; of the
        whole set: field_stats) and no percentiles (field_quantiles)."""
        return _range_facets(self, session.h if session is not None else self._default_session(), filter, field, edges)

    def last_range_stats(self, session=None):
        """(masks built, masks reused, k_range_counts launches) of the session's last range_facets device call."""
        return _u32_stats(self, "infx_engine_last_range_stats", session.h if session is not None else self._default_session(), 3)

    def field_stats(self, filter=None, field=None, group_by=None, session=None):
        """Field statistics (not in the reference): over the documents list_documents(filter) lists — not Deleted, their own fields accepted by `filter`; None:
        every live document; duplicate keys are documents of their own — the number of values of the int64 or double column `field` that are not a NaN, the
        NaNs, the smallest and largest value, and the EXACT sum and mean: an int column's sum is a Python int (it may exceed 64 bits), a double column's the
        exact real sum of the finite values rounded once to nearest-even (what math.fsum returns; beyond the double range +-inf; +inf / -inf / NaN with
        infinite members), the mean the exact sum / count rounded once.  The device adds integers only, so every run returns the same bytes.  With `group_by`
        (any column of at most 4096 distinct values, `field` itself included) the same figures for every group that has a member, members descending then value
        ascending, all of them.  Returns FieldStats(count, nan, total, min, max, sum, mean, groups, error).  A sequence of StatsRequest as first argument ->
        a list of FieldStats, sixteen requests per device call, all answered in ONE pass over the corpus; a request with a syntax error, MATCHES, a missing,
        unknown or string field, an unknown or too large group_by, or a double column that spans more than 128 binary digits gets `error` set, alone."""
        return _field_stats(self, session.h if session is not None else self._default_session(), filter, field, group_by)

    def last_field_stats_stats(self, session=None):
        """(masks built, masks reused, k_field_stats launches) of the session's last field_stats device call."""
        return _u32_stats(self, "infx_engine_last_field_stats_stats", session.h if session is not None else self._default_session(), 3)

    def bucket_stats(self, filter=None, field=None, bucket_by=None, edges=(), session=None):
        """Field statistics per range bucket (not in the reference): over the documents list_documents(filter) lists, the members are cut by their value of
        `bucket_by` into range_facets' half-open buckets [edges[i], edges[i + 1]), below edges[0], at or above edges[-1] and NaN — bucket_by and edges are
        range_facets' field and edges, under its rules — and every row carries field_stats' figures of `field` over its members: BucketRow(size, count, nan,
        min, max, sum, mean), size == count + nan, sum and mean EXACT as in field_stats (field_stats' `field`: an int64 or a double column of at most 128
        binary digits; it may be bucket_by itself); an empty row reads as field_stats on an empty set.  Returns BucketStats(edges, buckets, below, above, nan,
        whole, total, error): whole equals field_stats(filter, field) figure for figure, the rows' sizes are range_facets(filter, bucket_by, edges)' counts,
        nan.size + below.size + the buckets' sizes + above.size == total == whole.size, the rows' count / nan add up to whole's and on an int column so do
        the sums.  The device adds integers only: every run, session and rank returns the same bytes.  A sequence of BucketStatsRequest as first argument
        -> a list of BucketStats, sixteen requests per device call, all answered in ONE pass over the corpus; a request with a syntax error, MATCHES, a
        missing, unknown or string field, a field that cannot be summed exactly, a missing, unknown or string bucket_by or bad edges gets `error` set,
        alone.  Left out on purpose: a group_by beside the buckets, quantiles per bucket, automatic edges, a Query option."""
        return _bucket_stats(self, session.h if session is not None else self._default_session(), filter, field, bucket_by, edges)

    def last_bucket_stats_stats(self, session=None):
        """(masks built, masks reused, k_bucket_stats launches) of the session's last bucket_stats device call."""
        return _u32_stats(self, "infx_engine_last_bucket_stats_stats", session.h if session is not None else self._default_session(), 3)

    def last_bucket_stats_placement(self, session=None):
        """(requests with slots in a workgroup's LDS, in a CU's whole LDS, in global memory) of the session's last bucket_stats device call."""
        return _u32_stats(self, "infx_engine_last_bucket_stats_placement", session.h if session is not None else self._default_session(), 3)

    def field_quantiles(self, filter=None, field=None, q=(0.5,), group_by=None, session=None):
        """Exact medians and percentiles (not in the reference): over the documents field_stats(filter) counts — not Deleted, their own fields accepted by
        `filter`; None: every live document; duplicate keys are documents of their own — for every q[i] (1 .. 16 numbers in [0, 1], any order, duplicates
        allowed) the value at 0-based position floor((count - 1) * q[i]) of the non-NaN values of the int64 or double column `field` in ascending order: what
        numpy.quantile(method="lower") picks, never interpolated, always a value some member has (int for an int column, float for a double one; None when
        count == 0).  q = 0 is FieldStats.min, q = 1 FieldStats.max, and list_documents(filter, order_by=field, offset=nan + position, limit=1) lists a
        document of that value.  With `group_by` (any column of at most 4096 distinct values, `field` itself included) the same for every group that has a
        member, each at the positions of its own count, in FieldStats.groups' order.  Returns FieldQuantiles(q, values, count, nan, total, groups, error).
        The device selects on sort ranks with integer adds — all quantiles of all groups of all requests in the same few passes — so every run returns the
        same bytes.  A sequence of QuantileRequest as first argument -> a list of FieldQuantiles, sixteen requests per device call; a request with a syntax
        error, MATCHES, a missing, unknown or string field, an unknown or too large group_by, or no, more than 16 or out-of-range quantiles gets `error`
        set, alone.  Needs a GPU."""
        return _field_quantiles(self, session.h if session is not None else self._default_session(), filter, field, q, group_by)

    def last_field_quantiles_stats(self, session=None):
        """(masks built, masks reused, histogram passes, kernel launches) of the session's last field_quantiles device call."""
        return _u32_stats(self, "infx_engine_last_field_quantiles_stats", session.h if session is not None else self._default_session(), 4)

    def last_field_quantiles_placement(self, session=None):
        """(digit width, (request, pass) pairs with bins in LDS, pairs with bins in global memory) of the session's last field_quantiles device call."""
        return _u32_stats(self, "infx_engine_last_field_quantiles_placement", session.h if session is not None else self._default_session(), 3)

    def set_quantile_digit_bits(self, bits, session=None):
        """The width of a radix-select digit of field_quantiles on the session, 4 .. 11, or 0 (the default): chosen per call.  A tuning knob: it changes the
        number of passes, never an answer."""
        self._check(self.L.infx_engine_set_quantile_digit_bits(session.h if session is not None else self._default_session(), int(bits)))

    def _default_session(self):
        h = C.c_void_p(); self._check(self.L.infx_engine_default_session(self.h, C.byref(h))); return h

    def search_filtered(self, texts: Sequence[str], max_results=10, depth=500, enable_coverage=True, filter=None, enable_facets=False, session=None,
                        enable_boost=False, boosts=None, sort_by=None, sort_ascending=False, pre_filter=None):
        """Search(Query) with Query.Filter / Query.EnableFacets / Query.Boosts / Query.SortBy for a batch sharing them: post-filter, facet counts,
        boosts and sort-by run on the device (SearchEngine.ApplyPostProcessing order: filter, boosts, sort-by).  pre_filter: one Query.pre_filter
        for the whole batch (a query it cannot apply to comes back empty with Result.error set)."""
        sh = session.h if session is not None else self._default_session()
        nin = C.c_uint32(0)
        self._check(self.L.infx_engine_set_filter(sh, filter.encode() if filter is not None else None, int(enable_facets), C.byref(nin)))
        try:
            _set_boosts(self, sh, boosts, enable_boost)
            _set_sort(self, sh, sort_by, sort_ascending)
            nq = len(texts)
            pst = _install_prefilters(self, sh, [pre_filter] * nq) if pre_filter is not None else None
            arena, offs = pack_texts(texts)
            try:
                keys, scores, ties, counts, flags = (session or self).search_packed(arena, offs, max_results, depth, enable_coverage)
            except Exception:
                self.L.infx_engine_set_query_prefilters(sh, 0, None, None)
                raise
            inpre = _in_prefilter(self, sh, nq) if pre_filter is not None else None
            out = []
            for i in range(nq):
                recs = [ScoreEntry(float(scores[i, k]), int(keys[i, k]), int(ties[i, k])) for k in range(int(counts[i]))]
                rejected = pre_filter is not None and (pst[i] != 0 or bool(flags[i] & 16))
                facets = self.facets_of(sh, nq, i) if enable_facets and not rejected else None
                out.append(Result(recs, bool(flags[i] & 1), bool(flags[i] & 2), bool(flags[i] & 4), bool(flags[i] & 8), facets, int(nin.value),
                                  total_in_pre_filter=int(inpre[i]) if inpre is not None else 0,
                                  error=_query_error(self, sh, i, int(pst[i])) if rejected else None))
            return out
        finally:
            self.L.infx_engine_set_filter(sh, None, 0, None)
            self.L.infx_engine_set_boosts(sh, 0, None, None, 0)
            self.L.infx_engine_set_sort(sh, None, 0)

    def search_queries(self, queries: Sequence[Query], session=None) -> List[Result]:
        """Search(Query) for a batch of Query objects, each with its own MaxNumberOfRecordsToReturn, EnableCoverage, Filter, EnableFacets, Boosts and
        SortBy (infx_engine_set_query_options) and CoverageSetup (infx_engine_set_query_coverage): one device batch per CoverageDepth, results in
        input order.  A query whose options are refused (syntax error, MATCHES, more than 8 filtered boosts, post-processing on more than max_post_rows (default 64) rows,
        a CoverageSetup out of range or with the lexical pre-screen, a pre_filter that cannot apply) comes back empty with Result.error set; the others of
        the batch are unaffected.  Query.pre_filter (infx_engine_set_query_prefilters) is installed beside the options; a depth group is split further so
        that no device batch carries more than 16 distinct pre-filters."""
        sh = session.h if session is not None else self._default_session()
        runner = (session or self).search_packed
        out = [None] * len(queries)
        for depth, idx in _split_prefilters(queries, _by_depth(queries)):
            qs = [queries[i] for i in idx]
            status = _install_query_options(self, sh, qs)
            stride = max(1, max(int(q.max_number_of_records_to_return) for q in qs))
            arena, offs = pack_texts([q.text for q in qs])
            try:
                keys, scores, ties, counts, flags = runner(arena, offs, stride, depth, True)
            except Exception:
                _clear_query_options(self, sh)
                raise
            res = _query_results(self, sh, qs, status, keys, scores, ties, counts, flags)
            _attach_pre_filter_facets(self, sh, qs, res)
            for i, r in zip(idx, res):
                out[i] = r
        return out

    # ---- search ----
    def search(self, query: Union[Query, str], max_results: Optional[int] = None) -> Result:
        q = query if isinstance(query, Query) else Query(query, max_results or 10)
        if q.coverage_setup is not None or q.pre_filter is not None or q.collapse_by is not None or q.highlight:
            return self.search_queries([q])[0]
        if q.filter is not None or q.enable_facets or (q.enable_boost and q.boosts) or q.sort_by is not None:
            return self.search_filtered([q.text], q.max_number_of_records_to_return, q.coverage_depth, q.enable_coverage, q.filter, q.enable_facets,
                                        enable_boost=q.enable_boost, boosts=q.boosts, sort_by=q.sort_by, sort_ascending=q.sort_ascending)[0]
        return self.search_batch([q.text], q.max_number_of_records_to_return, q.coverage_depth, q.enable_coverage)[0]

    def last_count_stats(self, session=None):
        """(expressions the session's last per-query batch counted for NumberOfDocumentsInFilter, kernel launches it took)."""
        return _u32_stats(self, "infx_engine_last_count_stats", session.h if session is not None else self._default_session(), 2)

    def last_collapse_stats(self, session=None):
        """(queries with Query.collapse_by that were folded, k_collapse launches) of the session's last search: (k, 1), or (0, 0) for a batch without one."""
        return _u32_stats(self, "infx_engine_last_collapse_stats", session.h if session is not None else self._default_session(), 2)

    def last_highlight_stats(self, session=None):
        """(queries with Query.highlight that were highlighted, k_highlight launches) of the session's last search: (k, 1), or (0, 0) for a batch without one."""
        return _u32_stats(self, "infx_engine_last_highlight_stats", session.h if session is not None else self._default_session(), 2)

    def last_highlight_timings(self, session=None):
        """(k_highlight's milliseconds, bytes of highlight rows downloaded) of the session's last search."""
        return _highlight_timings(self, session.h if session is not None else self._default_session())

    def stored_text(self, document_index: int) -> str:
        """The stored text of one document (internal index): lower(normalize(IndexedText)), what Stage 2 and Query.highlight read; Highlight's offsets are
        UTF-16 units of it."""
        fn = self.L.infx_engine_document_text; fn.restype = C.c_int64
        n = fn(self.h, C.c_int64(int(document_index)), None, C.c_int64(0))
        if n < 0:
            self._check(1)
        buf = np.zeros(max(int(n), 1), np.uint16)
        if fn(self.h, C.c_int64(int(document_index)), _p(buf, C.c_uint16), C.c_int64(int(n))) != n:
            self._check(1)
        return buf[:n].tobytes().decode("utf-16-le", errors="surrogatepass")

    def last_prefilter_stats(self, session=None):
        """(masks built, masks taken from the session's cache, k_filter_mask_multi launches) of the session's last search (or prefilter_mask call)."""
        return _u32_stats(self, "infx_engine_last_prefilter_stats", session.h if session is not None else self._default_session(), 3)

    def prefilter_mask(self, expr: str, session=None) -> np.ndarray:
        """Parity tooling: the device's mask of a pre-filter expression, one byte per indexed document (1 = Deleted or not accepted) — built, or taken
        from the session's cache."""
        return _prefilter_mask(self, session.h if session is not None else self._default_session(), expr)

    def last_browse_stats(self, session=None):
        """(groups — distinct filter programs, counted ones included —, k_browse_scan launches) of the session's last batch that had a browse query."""
        g = C.c_uint32(0); n = C.c_uint32(0)
        self._check(self.L.infx_engine_last_browse_stats(session.h if session is not None else self._default_session(), C.byref(g), C.byref(n)))
        return int(g.value), int(n.value)

    def set_filter_cache_limit(self, n: int):
        """Bound of the engine's filter cache (compiled expressions + their counts), least recently used first."""
        self._check(self.L.infx_engine_set_filter_cache_limit(self.h, C.c_uint64(int(n))))

    def filter_cache_size(self) -> int:
        self.L.infx_engine_filter_cache_size.restype = C.c_int64
        return int(self.L.infx_engine_filter_cache_size(self.h))

    def search_batch_raw(self, texts: Sequence[str], max_results=10, depth=500, enable_coverage=True):
        arena, offs = pack_texts(texts)
        return self.search_packed(arena, offs, max_results, depth, enable_coverage)

    def search_packed(self, arena, offs, max_results=10, depth=500, enable_coverage=True):
        nq = len(offs) - 1
        keys = np.full((nq, max_results), -1, np.int64); scores = np.zeros((nq, max_results), np.float32)
        ties = np.zeros((nq, max_results), np.uint8); counts = np.zeros(nq, np.uint32); flags = np.zeros(nq, np.uint32)
        self._check(self.L.infx_engine_search_batch(self.h, nq, _p(arena, C.c_uint16), _p(offs, C.c_uint64), max_results, depth,
                                                    int(enable_coverage), _p(keys, C.c_int64), _p(scores, C.c_float),
                                                    _p(ties, C.c_uint8), _p(counts, C.c_uint32), _p(flags, C.c_uint32)))
        return keys, scores, ties, counts, flags

    def search_batch(self, texts: Sequence[str], max_results=10, depth=500, enable_coverage=True) -> List[Result]:
        keys, scores, ties, counts, flags = self.search_batch_raw(texts, max_results, depth, enable_coverage)
        out = []
        for i in range(len(texts)):
            recs = [ScoreEntry(float(scores[i, k]), int(keys[i, k]), int(ties[i, k])) for k in range(int(counts[i]))]
            out.append(Result(recs, bool(flags[i] & 1), bool(flags[i] & 2), bool(flags[i] & 4), bool(flags[i] & 8)))
        return out

    def last_timings(self):
        host = np.zeros(5, np.float64); kern = np.zeros(5, np.float32); alg = np.zeros(6, np.uint64)
        self._check(self.L.infx_engine_last_timings(self.h, _p(host, C.c_double), _p(kern, C.c_float), _p(alg, C.c_uint64)))
        return {"plan_ms": host[0], "stage1_ms": host[1], "prep2_ms": host[2], "stage2_ms": host[3], "post_ms": host[4],
                "k_accumulate_ms": float(kern[0]), "k_select_ms": float(kern[1]), "k_stage2_ms": float(kern[2]),
                "k_prep2_ms": float(kern[3]), "k_finalize_ms": float(kern[4]),
                "alg_bytes": int(alg[0]), "stage2_candidates": int(alg[1]), "stage2_text_bytes": int(alg[2]),
                "streamed_bytes": int(alg[3]), "stage1_candidates": int(alg[4]), "exact_replays": int(alg[5])}

    # ---- introspection (parity tests) ----
    def index_stats(self):
        n = C.c_int64(); t = C.c_int64(); p = C.c_int64(); a = C.c_float()
        self._check(self.L.infx_engine_index_stats(self.h, C.byref(n), C.byref(t), C.byref(p), C.byref(a)))
        return {"docs": n.value, "terms": t.value, "postings": p.value, "avgdl": a.value}

    def export_index(self):
        s = self.index_stats()
        T, P, N = s["terms"], s["postings"], s["docs"]
        df = np.zeros(T, np.int32); off = np.zeros(T + 1, np.uint64); pd = np.zeros(max(P, 1), np.int32)
        pw = np.zeros(max(P, 1), np.uint8); dl = np.zeros(max(N, 1), np.float32)
        self._check(self.L.infx_engine_export_index(self.h, _p(df, C.c_int32), _p(off, C.c_uint64), _p(pd, C.c_int32), _p(pw, C.c_uint8), _p(dl, C.c_float)))
        return {"df": df, "post_off": off, "post_doc": pd[:P], "post_w": pw[:P], "doc_len": dl[:N], "avgdl": s["avgdl"]}

    def term_text(self, t):
        buf = np.zeros(256, np.uint16)
        n = self.L.infx_engine_term_text(self.h, int(t), _p(buf, C.c_uint16), 256)
        return buf[:max(n, 0)].tobytes().decode("utf-16-le", errors="surrogatepass")

    def add_synonym(self, a, b):
        """SynonymMap.AddSynonym — before index_documents."""
        ua, ub = _u16(a), _u16(b)
        self._check(self.L.infx_engine_add_synonym(self.h, _p(ua, C.c_uint16), len(ua), _p(ub, C.c_uint16), len(ub)))

    def match_ld1_forward(self, q, cap=1024):
        a = _u16(q); out = np.zeros(cap, np.int32)
        c = self.L.infx_engine_match_ld1_forward(self.h, _p(a, C.c_uint16), len(a), _p(out, C.c_int32), cap)
        return c, out[:min(c, cap)].copy()

    def match_ld1(self, q, cap=1024):
        a = _u16(q); out = np.zeros(cap, np.int32)
        c = self.L.infx_engine_match_ld1(self.h, _p(a, C.c_uint16), len(a), _p(out, C.c_int32), cap)
        return c, out[:min(c, cap)].copy()

    def plan(self, text, depth=500, cap=256):
        a = _u16(text)
        t = np.zeros(cap, np.int32); df = np.zeros(cap, np.int32); idf = np.zeros(cap, np.float32)
        roles = np.zeros(cap, np.uint8); ranks = np.zeros(cap, np.uint8); meta = np.zeros(5, np.int32); flags = C.c_int32(0)
        n = self.L.infx_engine_plan(self.h, _p(a, C.c_uint16), len(a), depth, _p(t, C.c_int32), _p(df, C.c_int32), _p(idf, C.c_float),
                                    _p(roles, C.c_uint8), _p(ranks, C.c_uint8), cap, _p(meta, C.c_int32), C.byref(flags))
        return {"term_ids": t[:n].copy(), "df": df[:n].copy(), "idf": idf[:n].copy(), "roles": roles[:n].copy(), "ranks": ranks[:n].copy(),
                "mode": int(meta[0]), "prefix_set": int(meta[1]), "n_and": int(meta[2]), "df_s1": int(meta[3]), "df_s2": int(meta[4]),
                "flags": flags.value}

    def fuzzy_cache_size(self) -> int:
        """Entries of the LD1 expansion cache (LRU, at most 1000 like the reference's)."""
        self.L.infx_engine_fuzzy_cache_size.restype = C.c_int64
        return int(self.L.infx_engine_fuzzy_cache_size(self.h))

    def wordmatcher(self, text, cap=1 << 22):
        a = _u16(text); out = np.zeros(cap, np.int32)
        n = self.L.infx_engine_wordmatcher(self.h, _p(a, C.c_uint16), len(a), _p(out, C.c_int32), C.c_int64(cap))
        return out[:min(n, cap)].copy()

    # ---- the planning lookups as the device answers them (infidex_engine.h; tests/test_gpu_lookups.py) ----
    def device_lookups(self) -> bool:
        return self.L.infx_engine_device_lookups(self.h) == 1

    def lookup_stats(self):
        out = np.zeros(4, np.int64)
        self._check(self.L.infx_engine_lookup_stats(self.h, _p(out, C.c_int64)))
        return dict(ld1_device=int(out[0]), ld1_host=int(out[1]), wm_device=int(out[2]), wm_host=int(out[3]))

    def match_ld1_device(self, q, cap=1024):
        """(count, first `cap` term ids) like match_ld1; count -1 / -2: the kernel handed the word back to the host walk."""
        a = _u16(q); out = np.zeros(cap, np.int32)
        c = self.L.infx_engine_match_ld1_device(self.h, _p(a, C.c_uint16), len(a), _p(out, C.c_int32), cap)
        if c <= -100:
            self._check(-100 - c if c < -100 else 1)
        return c, out[:max(0, min(c, cap))].copy()

    def wordmatcher_device(self, text, cap=1 << 22):
        """Ascending unique doc ids of the lists k_wm emits for the (already prepared) search text; None: not admissible for the device lookup."""
        a = _u16(text); out = np.zeros(cap, np.int32)
        self.L.infx_engine_wordmatcher_device.restype = C.c_int64
        n = self.L.infx_engine_wordmatcher_device(self.h, _p(a, C.c_uint16), len(a), _p(out, C.c_int32), C.c_int64(cap))
        if n == -2:
            return None
        if n < 0:
            self._check(1)
        return out[:min(n, cap)].copy()

    def prefix_pop(self, p):
        a = _u16(p)
        return int(self.L.infx_engine_prefix_pop(self.h, _p(a, C.c_uint16), len(a)))

    def set_introspection(self, on=True):
        """Parity tooling: keep the Stage-1 rows / Stage-2 candidates of the last batch for last_stage1() / last_stage2()."""
        self._check(self.L.infx_engine_set_introspection(self.h, int(bool(on))))

    def last_stage1(self, qi, cap=4096):
        keys = np.zeros(cap, np.int64); sc = np.zeros(cap, np.float32)
        n = self.L.infx_engine_last_stage1(self.h, qi, _p(keys, C.c_int64), _p(sc, C.c_float), cap)
        n = max(n, 0)
        return keys[:n].copy(), sc[:n].copy()

    def last_stage2(self, cap=1 << 20):
        qo = np.zeros(cap, np.uint32); docs = np.zeros(cap, np.int32); base = np.zeros(cap, np.float32); sc = np.zeros(cap, np.float32)
        ties = np.zeros(cap, np.uint8); feat = np.zeros((cap, INFX_NFEAT), np.int32)
        n = self.L.infx_engine_last_stage2(self.h, _p(qo, C.c_uint32), _p(docs, C.c_int32), _p(base, C.c_float), _p(sc, C.c_float),
                                           _p(ties, C.c_uint8), _p(feat, C.c_int32), C.c_int64(cap))
        n = min(int(n), cap)
        return qo[:n].copy(), docs[:n].copy(), base[:n].copy(), sc[:n].copy(), ties[:n].copy(), feat[:n].copy()


class Session:
    """One in-flight batch (own HIP stream + scratch) on a SearchEngine; use one per host thread to overlap the host-side
    preparation of a batch with the GPU stages of another (infidex_engine.h)."""

    def __init__(self, engine: "SearchEngine"):
        self.engine = engine
        self.L = engine.L
        h = C.c_void_p()
        engine._check(self.L.infx_engine_session_create(engine.h, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.infx_engine_session_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def search_packed(self, arena, offs, max_results=10, depth=500, enable_coverage=True):
        nq = len(offs) - 1
        keys = np.full((nq, max_results), -1, np.int64); scores = np.zeros((nq, max_results), np.float32)
        ties = np.zeros((nq, max_results), np.uint8); counts = np.zeros(nq, np.uint32); flags = np.zeros(nq, np.uint32)
        self.engine._check(self.L.infx_engine_session_search_batch(self.h, nq, _p(arena, C.c_uint16), _p(offs, C.c_uint64), max_results, depth,
                                                                   int(enable_coverage), _p(keys, C.c_int64), _p(scores, C.c_float),
                                                                   _p(ties, C.c_uint8), _p(counts, C.c_uint32), _p(flags, C.c_uint32)))
        return keys, scores, ties, counts, flags

    def set_filter(self, expr=None, enable_facets=False):
        """Installs Query.Filter / Query.EnableFacets on this session (None clears); returns Filter.NumberOfDocumentsInFilter."""
        nin = C.c_uint32(0)
        self.engine._check(self.L.infx_engine_set_filter(self.h, expr.encode() if expr is not None else None, int(enable_facets), C.byref(nin)))
        return int(nin.value)

    def set_boosts(self, boosts=None, enable_boost=True):
        """Installs Query.Boosts (a sequence of Boost; None or enable_boost=False clears) on this session."""
        _set_boosts(self.engine, self.h, boosts, enable_boost)

    def search_queries(self, queries: Sequence[Query]) -> List[Result]:
        """SearchEngine.search_queries on this session."""
        return self.engine.search_queries(queries, session=self)

    def facets_of_all_documents(self):
        """SearchEngine.facets_of_all_documents on this session."""
        return _facets_all(self.engine, self.h)

    def facets_of_documents(self, filters):
        """SearchEngine.facets_of_documents on this session (the cached answers are the engine's)."""
        return _facets_filtered(self.engine, self.h, filters)

    def last_filtered_facet_stats(self):
        """SearchEngine.last_filtered_facet_stats of this session."""
        return _u32_stats(self.engine, "infx_engine_last_facets_filtered_stats", self.h, 3)

    def list_documents(self, filter=None, order_by=None, ascending=True, offset=0, limit=20):
        """SearchEngine.list_documents on this session (its mask cache holds the filters' masks)."""
        return _list_documents(self.engine, self.h, filter, order_by, ascending, offset, limit)

    def last_list_stats(self):
        """SearchEngine.last_list_stats of this session."""
        return _u32_stats(self.engine, "infx_engine_last_list_stats", self.h, 4)

    def set_list_digit_bits(self, bits):
        """The width of a radix-select digit of list_documents on this session, 4 .. 11 (default 11): a tuning knob, the pages do not depend on it."""
        self.engine._check(self.engine.L.infx_engine_set_list_digit_bits(self.h, int(bits)))

    def list_groups(self, filter=None, group_by=None, order_by=None, ascending=True, offset=0, limit=20):
        """SearchEngine.list_groups on this session (its mask cache holds the filters' masks)."""
        return _list_groups(self.engine, self.h, filter, group_by, order_by, ascending, offset, limit)

    def last_group_list_stats(self):
        """SearchEngine.last_group_list_stats of this session."""
        return _u32_stats(self.engine, "infx_engine_last_group_list_stats", self.h, 5)

    def list_group_members(self, filter=None, group_by=None, order_by=None, ascending=True, per_group=3, offset=0, limit=20):
        """SearchEngine.list_group_members on this session (its mask cache holds the filters' masks)."""
        return _list_group_members(self.engine, self.h, filter, group_by, order_by, ascending, per_group, offset, limit)

    def last_group_members_stats(self):
        """SearchEngine.last_group_members_stats of this session."""
        return _u32_stats(self.engine, "infx_engine_last_group_members_stats", self.h, 6)

    def top_groups(self, filter=None, group_by=None, by="size", field=None, ascending=False, offset=0, limit=20):
        """SearchEngine.top_groups on this session (its mask cache holds the filters' masks)."""
        return _top_groups(self.engine, self.h, filter, group_by, by, field, ascending, offset, limit)

    def last_top_groups_stats(self):
        """SearchEngine.last_top_groups_stats of this session."""
        return _u32_stats(self.engine, "infx_engine_last_top_groups_stats", self.h, 5)

    def last_top_groups_placement(self):
        """SearchEngine.last_top_groups_placement of this session."""
        return _u32_stats(self.engine, "infx_engine_last_top_groups_placement", self.h, 3)

    def field_distinct(self, filter=None, field=None, group_by=None):
        """SearchEngine.field_distinct on this session (its mask cache holds the filters' masks)."""
        return _field_distinct(self.engine, self.h, filter, field, group_by)

    def last_field_distinct_stats(self):
        """SearchEngine.last_field_distinct_stats of this session."""
        return _u32_stats(self.engine, "infx_engine_last_field_distinct_stats", self.h, 6)

    def set_distinct_placement(self, mode):
        """SearchEngine.set_distinct_placement of this session."""
        self.engine._check(self.engine.L.infx_engine_set_distinct_placement(self.h, int(mode)))

    def range_facets(self, filter=None, field=None, edges=()):
        """SearchEngine.range_facets on this session (its mask cache holds the filters' masks)."""
        return _range_facets(self.engine, self.h, filter, field, edges)

    def last_range_stats(self):
        """SearchEngine.last_range_stats of this session."""
        return _u32_stats(self.engine, "infx_engine_last_range_stats", self.h, 3)

    def field_stats(self, filter=None, field=None, group_by=None):
        """SearchEngine.field_stats on this session (its mask cache holds the filters' masks)."""
        return _field_stats(self.engine, self.h, filter, field, group_by)

    def last_field_stats_stats(self):
        """SearchEngine.last_field_stats_stats of this session."""
        return _u32_stats(self.engine, "infx_engine_last_field_stats_stats", self.h, 3)

    def bucket_stats(self, filter=None, field=None, bucket_by=None, edges=()):
        """SearchEngine.bucket_stats on this session (its mask cache holds the filters' masks)."""
        return _bucket_stats(self.engine, self.h, filter, field, bucket_by, edges)

    def last_bucket_stats_stats(self):
        """SearchEngine.last_bucket_stats_stats of this session."""
        return _u32_stats(self.engine, "infx_engine_last_bucket_stats_stats", self.h, 3)

    def last_bucket_stats_placement(self):
        """SearchEngine.last_bucket_stats_placement of this session."""
        return _u32_stats(self.engine, "infx_engine_last_bucket_stats_placement", self.h, 3)

    def field_quantiles(self, filter=None, field=None, q=(0.5,), group_by=None):
        """SearchEngine.field_quantiles on this session (its mask cache holds the filters' masks)."""
        return _field_quantiles(self.engine, self.h, filter, field, q, group_by)

    def last_field_quantiles_stats(self):
        """SearchEngine.last_field_quantiles_stats of this session."""
        return _u32_stats(self.engine, "infx_engine_last_field_quantiles_stats", self.h, 4)

    def last_field_quantiles_placement(self):
        """SearchEngine.last_field_quantiles_placement of this session."""
        return _u32_stats(self.engine, "infx_engine_last_field_quantiles_placement", self.h, 3)

    def set_quantile_digit_bits(self, bits):
        """SearchEngine.set_quantile_digit_bits of this session."""
        self.engine._check(self.engine.L.infx_engine_set_quantile_digit_bits(self.h, int(bits)))

    def last_collapse_stats(self):
        """SearchEngine.last_collapse_stats of this session."""
        return _u32_stats(self.engine, "infx_engine_last_collapse_stats", self.h, 2)

    def last_highlight_stats(self):
        """SearchEngine.last_highlight_stats of this session."""
        return _u32_stats(self.engine, "infx_engine_last_highlight_stats", self.h, 2)

    def last_highlight_timings(self):
        """SearchEngine.last_highlight_timings of this session."""
        return _highlight_timings(self.engine, self.h)

    def last_prefilter_stats(self):
        """SearchEngine.last_prefilter_stats of this session."""
        return _u32_stats(self.engine, "infx_engine_last_prefilter_stats", self.h, 3)

    def prefilter_mask(self, expr: str) -> np.ndarray:
        """SearchEngine.prefilter_mask on this session (its own mask cache)."""
        return _prefilter_mask(self.engine, self.h, expr)

    def last_count_stats(self):
        """(expressions the last per-query batch counted for NumberOfDocumentsInFilter, kernel launches it took)."""
        return _u32_stats(self.engine, "infx_engine_last_count_stats", self.h, 2)

    def set_sort(self, sort_by=None, ascending=False):
        """Installs Query.SortBy (a field name; None = relevance order) and Query.SortAscending on this session."""
        _set_sort(self.engine, self.h, sort_by, ascending)

    def last_timings(self, kernels=True):
        """Host phase times of the session's last batch; kernels=True adds the kernel durations (HIP events on the session's stream).  Resolving those costs a
        handful of HIP API calls, which queue behind the launches of other sessions: a throughput run asks for them on a sample of its batches only."""
        host = np.zeros(5, np.float64); kern = np.zeros(5, np.float32); alg = np.zeros(6, np.uint64)
        self.engine._check(self.L.infx_engine_session_last_timings(self.h, _p(host, C.c_double), _p(kern, C.c_float) if kernels else None, _p(alg, C.c_uint64)))
        pb = np.zeros(4, np.float64)
        self.engine._check(self.L.infx_engine_session_plan_breakdown(self.h, _p(pb, C.c_double)))
        out = {"plan_ms": host[0], "stage1_ms": host[1], "prep2_ms": host[2], "stage2_ms": host[3], "post_ms": host[4],
               "plan_tokens_ms": float(pb[0]), "plan_ld1_device_ms": float(pb[1]), "plan_union_device_ms": float(pb[2]), "plan_finish_ms": float(pb[3]),
               "alg_bytes": int(alg[0]), "stage2_candidates": int(alg[1]), "stage2_text_bytes": int(alg[2]),
               "streamed_bytes": int(alg[3]), "stage1_candidates": int(alg[4]), "exact_replays": int(alg[5])}
        if kernels:
            rms = C.c_float(0); why = np.zeros(3, np.uint32); parts = np.zeros(4, np.float32)
            self.engine._check(self.L.infx_engine_session_last_replay(self.h, C.byref(rms), _p(why, C.c_uint32)))
            self.engine._check(self.L.infx_engine_session_replay_breakdown(self.h, _p(parts, C.c_float)))
            out.update({"k_replay_ms": float(rms.value), "flag_plateau": int(why[0]), "flag_band": int(why[1]), "flag_unknown": int(why[2]),
                        "k_ex_scan_ms": float(parts[0]), "k_ex_chunk_ms": float(parts[1]), "k_ex_heap_ms": float(parts[2]), "k_exact1_ms": float(parts[3]),
                        "k_accumulate_ms": float(kern[0]), "k_select_ms": float(kern[1]), "k_stage2_ms": float(kern[2]),
                        "k_prep2_ms": float(kern[3]), "k_finalize_ms": float(kern[4])})
            clp = np.zeros(2, np.float32)      # a batch with Query.collapse_by: k_finalize alone and k_collapse (k_finalize_ms spans both and the post-processing)
            self.engine._check(self.L.infx_engine_last_collapse_timings(self.h, _p(clp, C.c_float)))
            out.update({"k_finalize_rows_ms": float(clp[0]), "k_collapse_ms": float(clp[1])})
        return out


def _set_boosts(engine, sh, boosts, enable_boost):
    """infx_engine_set_boosts: Query.EnableBoost + Query.Boosts on session handle sh (boosts with filter None are passed as NULL and dropped there)."""
    bs = list(boosts) if boosts else []
    on = bool(enable_boost) and len(bs) > 0
    exprs = (C.c_char_p * max(len(bs), 1))(*[b.filter.encode() if b.filter is not None else None for b in bs])
    st = np.asarray([int(b.strength) for b in bs] or [0], np.int32)
    engine._check(engine.L.infx_engine_set_boosts(sh, len(bs) if on else 0, exprs, _p(st, C.c_int32), int(on)))


class _QueryOptions(C.Structure):      # infx_query_options (include/infidex_engine.h)
    _fields_ = [("max_results", C.c_int32), ("enable_coverage", C.c_int32), ("enable_facets", C.c_int32), ("enable_boost", C.c_int32),
                ("filter", C.c_char_p), ("nboosts", C.c_uint32), ("boost_filters", C.POINTER(C.c_char_p)), ("boost_strengths", C.POINTER(C.c_int32)),
                ("sort_by", C.c_char_p), ("sort_ascending", C.c_int32)]


def _by_depth(queries):
    """[(CoverageDepth, [indices in input order])]: one device batch per depth."""
    groups = {}
    for i, q in enumerate(queries):
        groups.setdefault(int(q.coverage_depth), []).append(i)
    return list(groups.items())


MAX_PREFILTERS = 16      # INFX_MAX_PREFILTERS: distinct pre-filters one device batch can carry


def _split_prefilters(queries, groups, limit=MAX_PREFILTERS):
    """Splits each (depth, [indices]) group further, keeping input order, so that no group holds more than `limit` distinct Query.pre_filter expressions."""
    out = []
    for depth, idx in groups:
        cur, seen = [], set()
        for i in idx:
            p = queries[i].pre_filter
            if p is not None and p not in seen and len(seen) >= limit:
                out.append((depth, cur)); cur, seen = [], set()
            if p is not None:
                seen.add(p)
            cur.append(i)
        if cur:
            out.append((depth, cur))
    return out


def _install_prefilters(engine, sh, exprs):
    """infx_engine_set_query_prefilters for the coming batch on session handle sh (None entries: no pre-filter); returns each query's status."""
    n = len(exprs)
    arr = (C.c_char_p * max(n, 1))(*[x.encode() if x is not None else None for x in exprs])
    st = np.zeros(max(n, 1), np.int32)
    engine._check(engine.L.infx_engine_set_query_prefilters(sh, n, arr, _p(st, C.c_int32)))
    return st[:n]


def _in_prefilter(engine, sh, n):
    out = np.zeros(max(n, 1), np.uint32)
    engine._check(engine.L.infx_engine_last_in_prefilter(sh, n, _p(out, C.c_uint32)))
    return out[:n]


def _request_error(engine, fn, sh, i, status):
    """The message the library's reader fn has for request (or query) i of the session's last call; "status <n>" when it has none."""
    buf = C.create_string_buffer(512); getattr(engine.L, fn)(sh, i, buf, 512)
    return buf.value.decode(errors="replace") or ("status %d" % status)


def _query_error(engine, sh, j, status):
    return _request_error(engine, "infx_engine_query_error", sh, j, status)


def _u32_stats(engine, fn, sh, k):
    """The k uint32 counters the library's getter fn reports for session handle sh."""
    v = [C.c_uint32(0) for _ in range(k)]
    engine._check(getattr(engine.L, fn)(sh, *[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def _prefilter_mask(engine, sh, expr):
    n = int(engine.index_stats()["docs"])
    out = np.zeros(max(n, 1), np.uint8)
    engine._check(engine.L.infx_engine_prefilter_mask(sh, expr.encode(), _p(out, C.c_uint8), C.c_uint64(len(out))))
    return out[:n]


def _install_query_options(engine, sh, qs):
    """infx_engine_set_query_options for the queries qs on session handle sh; returns each query's status (0: accepted)."""
    n = len(qs)
    arr = (_QueryOptions * max(n, 1))()
    keep = []
    for o, q in zip(arr, qs):
        o.max_results = int(q.max_number_of_records_to_return); o.enable_coverage = int(bool(q.enable_coverage))
        o.enable_facets = int(bool(q.enable_facets)); o.enable_boost = int(bool(q.enable_boost))
        o.filter = q.filter.encode() if q.filter is not None else None
        bs = list(q.boosts) if q.boosts else []
        if bs:
            ex = (C.c_char_p * len(bs))(*[b.filter.encode() if b.filter is not None else None for b in bs])
            st = (C.c_int32 * len(bs))(*[int(b.strength) for b in bs])
            keep += [ex, st]
            o.nboosts = len(bs); o.boost_filters = C.cast(ex, C.POINTER(C.c_char_p)); o.boost_strengths = C.cast(st, C.POINTER(C.c_int32))
        o.sort_by = q.sort_by.encode() if q.sort_by is not None else None; o.sort_ascending = int(bool(q.sort_ascending))
    status = np.zeros(max(n, 1), np.int32)
    engine._check(engine.L.infx_engine_set_query_options(sh, n, arr, _p(status, C.c_int32)))
    status = status[:n]
    # the other parts, installed beside the options and consumed by the same batch, in the library's fixed order: (what a query asks of it, install it, clear it)
    L = engine.L
    parts = ((lambda q: q.coverage_setup, lambda: _install_coverage(engine, sh, qs), lambda: L.infx_engine_set_query_coverage(sh, 0, None, None)),
             (lambda q: q.pre_filter, lambda: _install_prefilters(engine, sh, [q.pre_filter for q in qs]), lambda: L.infx_engine_set_query_prefilters(sh, 0, None, None)),
             (lambda q: q.collapse_by, lambda: _install_collapse(engine, sh, qs), lambda: L.infx_engine_set_query_collapse(sh, 0, None, None, None)),
             (lambda q: True if q.highlight else None, lambda: _install_highlight(engine, sh, qs), lambda: L.infx_engine_set_query_highlight(sh, 0, None, None)))
    for asked, install, clear in parts:
        if not any(asked(q) is not None for q in qs):
            engine._check(clear())
            continue
        try:
            st = install()
        except Exception:
            _clear_query_options(engine, sh)
            raise
        status = np.where(status != 0, status, st)
    return status


def _install_coverage(engine, sh, qs):
    """infx_engine_set_query_coverage for the coming batch on session handle sh (Query.CoverageSetup None: the engine's); returns each query's status."""
    n = len(qs)
    sts = [_coverage_struct(q.coverage_setup) if q.coverage_setup is not None else None for q in qs]
    ptrs = (C.POINTER(_CoverageSetup) * max(n, 1))(*[C.pointer(st) if st is not None else None for st in sts])
    cst = np.zeros(max(n, 1), np.int32)
    engine._check(engine.L.infx_engine_set_query_coverage(sh, n, ptrs, _p(cst, C.c_int32)))
    return cst[:n]


def _install_collapse(engine, sh, qs):
    """infx_engine_set_query_collapse for the coming batch on session handle sh (Query.collapse_by None: not collapsed); returns each query's status."""
    n = len(qs)
    arr = (C.c_char_p * max(n, 1))(*[str(q.collapse_by).encode() if q.collapse_by is not None else None for q in qs])
    keeps = np.asarray([min(max(int(q.collapse_keep), -1), 2 ** 31 - 1) for q in qs] or [1], np.int32)
    st = np.zeros(max(n, 1), np.int32)
    engine._check(engine.L.infx_engine_set_query_collapse(sh, n, arr, _p(keeps, C.c_int32), _p(st, C.c_int32)))
    return st[:n]


def _attach_collapse(engine, sh, qs, results):
    """Result.group_values / group_sizes / total_groups / total_ranked of the queries of a batch just searched on session handle sh that ran with collapse_by."""
    n = len(qs)
    if not any(q.collapse_by is not None and r.error is None for q, r in zip(qs, results)):
        return
    groups = np.zeros(max(n, 1), np.uint32); ranked = np.zeros(max(n, 1), np.uint32)
    engine._check(engine.L.infx_engine_last_collapse(sh, n, _p(groups, C.c_uint32), _p(ranked, C.c_uint32)))
    texts = _value_texts(engine)
    for j, (q, r) in enumerate(zip(qs, results)):
        if q.collapse_by is None or r.error is not None:
            continue
        m = len(r.records); col = C.c_int32(-1)
        codes = np.zeros(max(m, 1), np.uint32); sizes = np.zeros(max(m, 1), np.uint32)
        got = engine.L.infx_engine_collapse_rows(sh, j, C.byref(col), _p(codes, C.c_uint32), _p(sizes, C.c_uint32), m)
        if got != m:
            engine._check(1 if got < 0 else 0)
            raise InfidexError(1, "collapse_by: %d rows described, %d returned" % (got, m))
        r.group_values = texts(str(q.collapse_by), codes[:m]); r.group_sizes = [int(x) for x in sizes[:m]]
        r.total_groups = int(groups[j]); r.total_ranked = int(ranked[j])


def _install_highlight(engine, sh, qs):
    """infx_engine_set_query_highlight for the coming batch on session handle sh (Query.highlight False: width 0, not asked); returns each query's status."""
    n = len(qs)
    # (a width of 0 would read as "not asked": an asking query's width is sent as given, 0 as -1, and refused by the library with the others out of range)
    chars = np.asarray([(min(max(int(q.highlight_chars), -1), 2 ** 31 - 1) or -1) if q.highlight else 0 for q in qs] or [0], np.int32)
    st = np.zeros(max(n, 1), np.int32)
    engine._check(engine.L.infx_engine_set_query_highlight(sh, n, _p(chars, C.c_int32), _p(st, C.c_int32)))
    return st[:n]


def _highlight_timings(engine, sh):
    ms = C.c_float(0); nbytes = C.c_uint64(0)
    engine._check(engine.L.infx_engine_last_highlight_timings(sh, C.byref(ms), C.byref(nbytes)))
    return float(ms.value), int(nbytes.value)


def _u16_text(a):
    return np.ascontiguousarray(a, np.uint16).tobytes().decode("utf-16-le", errors="surrogatepass")


def _attach_highlights(engine, sh, qs, results):
    """Result.highlights of the queries of a batch just searched on session handle sh that ran with Query.highlight: the rows k_highlight wrote (layout:
    csrc/highlight.h), one Highlight per returned row."""
    L = engine.L
    for j, (q, r) in enumerate(zip(qs, results)):
        if not q.highlight or r.error is not None:
            continue
        m = len(r.records)
        rows = C.c_int32(0); ts = C.c_int32(0); ss = C.c_int32(0); lq = C.c_int32(0); tl = C.c_int32(0); nw = C.c_int32(0)
        text = np.zeros(512, np.uint16); woff = np.zeros(32, np.uint16); wlen = np.zeros(32, np.uint16)
        if m == 0:
            r.highlights = []
            continue
        engine._check(L.infx_engine_highlight_query(sh, j, C.byref(rows), C.byref(ts), C.byref(ss), C.byref(lq), _p(text, C.c_uint16), C.byref(tl),
                                                    _p(woff, C.c_uint16), _p(wlen, C.c_uint16), C.byref(nw)))
        T, W = int(ts.value), int(ss.value)
        row_u16 = 10 + 8 * T + 5 * HIGHLIGHT_MAX_SPANS + W
        buf = np.zeros(max(m, 1) * row_u16, np.uint16)
        got = L.infx_engine_highlight_rows(sh, j, _p(buf, C.c_uint16), C.c_int64(len(buf)))
        if got != m:
            engine._check(1 if got < 0 else 0)
            raise InfidexError(1, "highlight: %d rows described, %d returned" % (got, m))
        words = [_u16_text(text[int(woff[k]):int(woff[k]) + int(wlen[k])]) for k in range(int(nw.value))]
        out = []
        for k in range(m):
            R = buf[k * row_u16:(k + 1) * row_u16]
            h = Highlight(HIGHLIGHT_STATUS[int(R[0])], int(R[6]) | (int(R[7]) << 16))
            if h.status == "ok":
                nt, ns = int(R[1]), int(R[2])
                h.truncated = bool(R[3]); h.snippet_start = int(R[4]); h.words = int(R[8])
                for i in range(nt):
                    t = R[10 + 8 * i:18 + 8 * i]
                    h.terms.append(TermMatch(words[i], HIGHLIGHT_KINDS[int(t[0])], int(t[2]), int(t[3]), int(t[4]), int(t[5]), int(t[1]), int(t[6]), int(t[7])))
                sp = R[10 + 8 * T:10 + 8 * T + 5 * ns].reshape(ns, 5)
                h.spans = [tuple(int(x) for x in s) for s in sp]
                at = 10 + 8 * T + 5 * HIGHLIGHT_MAX_SPANS
                h.snippet = _u16_text(R[at:at + int(R[5])])
            out.append(h)
        r.highlights = out


def _clear_query_options(engine, sh):
    """Drops the per-query options and coverage setups installed on session handle sh (a batch that failed before it consumed them)."""
    engine.L.infx_engine_set_query_options(sh, 0, None, None)
    engine.L.infx_engine_set_query_coverage(sh, 0, None, None)
    engine.L.infx_engine_set_query_prefilters(sh, 0, None, None)
    engine.L.infx_engine_set_query_collapse(sh, 0, None, None, None)
    engine.L.infx_engine_set_query_highlight(sh, 0, None, None)


def _query_results(engine, sh, qs, status, keys, scores, ties, counts, flags):
    """The Results of a per-query batch just searched on session handle sh."""
    n = len(qs)
    inf = np.zeros(max(n, 1), np.uint32)
    engine._check(engine.L.infx_engine_last_in_filter(sh, n, _p(inf, C.c_uint32)))
    inpre = _in_prefilter(engine, sh, n) if any(q.pre_filter is not None for q in qs) else None
    out = []
    for j, q in enumerate(qs):
        err = None
        # (a pre-filter on a browse query is refused when the batch runs: result flag bit 4 without an install status)
        if status[j] != 0 or ((q.pre_filter is not None or q.collapse_by is not None or q.highlight) and flags[j] & 16):
            err = _query_error(engine, sh, j, int(status[j]) or 5)
        recs = [ScoreEntry(float(scores[j, k]), int(keys[j, k]), int(ties[j, k])) for k in range(int(counts[j]))]
        facets = engine.facets_of(sh, n, j) if q.enable_facets and err is None else None
        out.append(Result(recs, bool(flags[j] & 1), bool(flags[j] & 2), bool(flags[j] & 4), bool(flags[j] & 8), facets, int(inf[j]),
                          total_in_pre_filter=int(inpre[j]) if inpre is not None else 0, error=err))
    _attach_collapse(engine, sh, qs, out)
    _attach_highlights(engine, sh, qs, out)
    return out


def _facets_all(engine, sh):
    ncols = C.c_int32(0)
    engine._check(engine.L.infx_engine_facets_all(sh, C.byref(ncols)))
    facets = _facet_columns(engine, int(ncols.value), lambda k, *out: engine.L.infx_engine_facets_all_column(sh, k, *out))
    facets.update(_facet_columns(engine, int(engine.L.infx_engine_facets_all_list_column_count(sh)),
                                 lambda k, *out: engine.L.infx_engine_facets_all_list_column(sh, k, *out), lists=True))
    return facets


def _list_column_index(engine, name):
    """(the engine's list column of a field name, the kind of its elements), or (-1, 0)."""
    for lcol in range(int(engine.L.infx_engine_list_column_count(engine.h))):
        nb = C.create_string_buffer(256); kind = C.c_int32(0)
        engine.L.infx_engine_list_column_info(engine.h, lcol, nb, 256, None, None, C.byref(kind))
        if nb.value and nb.value.decode() == name:
            return lcol, int(kind.value)
    return -1, 0


def _list_column_value(engine, lcol, code):
    n = int(engine.L.infx_engine_list_column_value(engine.h, lcol, code, None, 0))
    vb = C.create_string_buffer(max(n, 0) + 1); engine.L.infx_engine_list_column_value(engine.h, lcol, code, vb, n + 1)
    return vb.value.decode()


def _column_facets(engine, col, m, codes, cnts):
    """(field name, [(value, count)]) of m (code, count) pairs of engine column col."""
    nb = C.create_string_buffer(256); engine.L.infx_engine_column_info(engine.h, col, nb, 256, None, None)
    vals = []
    for j in range(m):
        vb = C.create_string_buffer(1024); engine.L.infx_engine_column_value(engine.h, col, int(codes[j]), vb, 1024)
        vals.append((vb.value.decode(), int(cnts[j])))
    return nb.value.decode(), vals


def _facet_columns(engine, ncols, read, lists=False):
    """{field: [(value, count)]} of ncols facet columns; read(k, col, codes, counts, cap) is the library's reader of the k-th: the number of pairs, < 0 for an error.
    lists: the columns are list columns (their own index space and name / value readers)."""
    facets = {}
    for k in range(ncols):
        col = C.c_int32(0); codes = np.zeros(128, np.uint32); cnts = np.zeros(128, np.uint32)
        m = read(k, C.byref(col), _p(codes, C.c_uint32), _p(cnts, C.c_uint32), 128)
        if m < 0:
            engine._check(1)
        if m > 0 and lists:
            nb = C.create_string_buffer(256); engine.L.infx_engine_list_column_info(engine.h, col.value, nb, 256, None, None, None)
            facets[nb.value.decode()] = [(_list_column_value(engine, col.value, int(codes[j])), int(cnts[j])) for j in range(m)]
        elif m > 0:
            name, vals = _column_facets(engine, col.value, m, codes, cnts)
            facets[name] = vals
    return facets


def _per_request(engine, sh, fn, error_fn, ctype, reqs, single, pack, read, refused, chunk=MAX_PREFILTERS):
    """The call pattern of the features that answer each request on its own, on session handle sh: reqs go to the library function fn `chunk` at a time
    (None: in one call, which the engine splits itself), as an array of ctype made by pack(request).  A request the engine refused becomes refused(request,
    message), the message from the library's reader error_fn; any other becomes read(i, request), i its place in the call.  One answer for `single`, else their list."""
    out = []
    for r0 in range(0, len(reqs), chunk) if chunk else [0]:
        part = reqs[r0:r0 + chunk] if chunk else reqs
        n = len(part)
        arr = (ctype * max(n, 1))(*[pack(r) for r in part])
        st = np.zeros(max(n, 1), np.int32)
        engine._check(getattr(engine.L, fn)(sh, n, arr, _p(st, C.c_int32)))
        for i, r in enumerate(part):
            out.append(refused(r, _request_error(engine, error_fn, sh, i, int(st[i]))) if st[i] != 0 else read(i, r))
    return out[0] if single else out


def _facets_filtered(engine, sh, filters):
    """infx_engine_facets_filtered on session handle sh: a FilteredFacets for a str, a list of them for a sequence."""
    def read(i, _):
        tot = C.c_uint32(0)
        engine._check(engine.L.infx_engine_facets_filtered_total(sh, i, C.byref(tot)))
        ncols = int(engine.L.infx_engine_facets_filtered_column_count(sh))
        facets = _facet_columns(engine, ncols, lambda k, *out: engine.L.infx_engine_facets_filtered_column(sh, i, k, *out))
        facets.update(_facet_columns(engine, int(engine.L.infx_engine_facets_filtered_list_column_count(sh)),
                                     lambda k, *out: engine.L.infx_engine_facets_filtered_list_column(sh, i, k, *out), lists=True))
        return FilteredFacets(facets, int(tot.value), None)
    single = isinstance(filters, str)
    return _per_request(engine, sh, "infx_engine_facets_filtered", "infx_engine_facets_filtered_error", C.c_char_p, [filters] if single else list(filters), single,
                        lambda x: x.encode(), read, lambda _, msg: FilteredFacets({}, 0, msg), chunk=None)


def _column_index(engine, name):
    """The engine's column of a field name, or -1."""
    for col in range(int(engine.L.infx_engine_column_count(engine.h))):
        nb = C.create_string_buffer(256); engine.L.infx_engine_column_info(engine.h, col, nb, 256, None, None)
        if nb.value.decode() == name:
            return col
    return -1


def _list_documents(engine, sh, filter, order_by, ascending, offset, limit):
    """infx_engine_list_documents on session handle sh: a Listing for one request (given by its parts), a list of them for a sequence of ListRequest."""
    def pack(r):
        off, lim = int(r.offset), int(r.limit)
        # out of the C fields' range: passed as values the engine refuses for this request alone
        return _ListReq(None if r.filter is None else r.filter.encode(), None if r.order_by is None else r.order_by.encode(), 1 if r.ascending else 0,
                        off if 0 <= off < 2 ** 32 else 0xFFFFFFFF, lim if 0 <= lim < 2 ** 32 else 0)
    cols = {}

    def read(i, r):
        tot = C.c_uint32(0)
        engine._check(engine.L.infx_engine_list_total(sh, i, C.byref(tot)))
        keys = np.zeros(1024, np.int64); docs = np.zeros(1024, np.int32); codes = np.zeros(1024, np.uint32)
        m = engine.L.infx_engine_list_rows(sh, i, _p(keys, C.c_int64), _p(docs, C.c_int32), _p(codes, C.c_uint32), 1024)
        if m < 0:
            engine._check(1)
        vals = []
        if r.order_by is not None:
            if r.order_by not in cols:
                cols[r.order_by] = (_column_index(engine, r.order_by), {})
            col, text = cols[r.order_by]
            for c in codes[:m]:
                c = int(c)
                if c not in text:
                    vb = C.create_string_buffer(1024); engine.L.infx_engine_column_value(engine.h, col, c, vb, 1024)
                    text[c] = vb.value.decode()
                vals.append(text[c])
        return Listing([int(k) for k in keys[:m]], vals, int(tot.value), None)
    single = filter is None or isinstance(filter, str)
    # (one mask slot per distinct filter: sixteen requests per device call)
    return _per_request(engine, sh, "infx_engine_list_documents", "infx_engine_list_error", _ListReq,
                        [ListRequest(filter, order_by, ascending, offset, limit)] if single else list(filter), single, pack, read,
                        lambda _, msg: Listing([], [], 0, msg))


def _value_texts(engine):
    """texts(name, codes): the values of column `name` at codes, as list_documents fetches them; every (column, code) is fetched once per call of this."""
    cols = {}

    def texts(name, codes):
        if name not in cols:
            cols[name] = (_column_index(engine, name), {})
        col, text = cols[name]
        out = []
        for c in codes:
            c = int(c)
            if c not in text:
                vb = C.create_string_buffer(1024); engine.L.infx_engine_column_value(engine.h, col, c, vb, 1024)
                text[c] = vb.value.decode()
            out.append(text[c])
        return out
    return texts


def _list_groups(engine, sh, filter, group_by, order_by, ascending, offset, limit):
    """infx_engine_list_groups on session handle sh: a GroupListing for one request (given by its parts), a list of them for a sequence of GroupListRequest."""
    def pack(r):
        off, lim = int(r.offset), int(r.limit)
        # out of the C fields' range: passed as values the engine refuses for this request alone
        return _GroupListReq(None if r.filter is None else r.filter.encode(), None if r.group_by is None else str(r.group_by).encode(),
                             None if r.order_by is None else r.order_by.encode(), 1 if r.ascending else 0,
                             off if 0 <= off < 2 ** 32 else 0xFFFFFFFF, lim if 0 <= lim < 2 ** 32 else 0)
    texts = _value_texts(engine)

    def read(i, r):
        groups = C.c_uint32(0); tot = C.c_uint32(0)
        engine._check(engine.L.infx_engine_group_list_totals(sh, i, C.byref(groups), C.byref(tot)))
        keys = np.zeros(1024, np.int64); docs = np.zeros(1024, np.int32); codes = np.zeros(1024, np.uint32); gcodes = np.zeros(1024, np.uint32); sizes = np.zeros(1024, np.uint32)
        m = engine.L.infx_engine_group_list_rows(sh, i, _p(keys, C.c_int64), _p(docs, C.c_int32), _p(codes, C.c_uint32), _p(gcodes, C.c_uint32), _p(sizes, C.c_uint32), 1024)
        if m < 0:
            engine._check(1)
        vals = [] if r.order_by is None else texts(r.order_by, codes[:m])
        return GroupListing([int(k) for k in keys[:m]], vals, texts(str(r.group_by), gcodes[:m]), [int(x) for x in sizes[:m]], int(groups.value), int(tot.value), None)
    single = filter is None or isinstance(filter, str)
    # (one mask slot per distinct filter: sixteen requests per device call)
    return _per_request(engine, sh, "infx_engine_list_groups", "infx_engine_group_list_error", _GroupListReq,
                        [GroupListRequest(filter, group_by, order_by, ascending, offset, limit)] if single else list(filter), single, pack, read,
                        lambda _, msg: GroupListing(error=msg))


def _list_group_members(engine, sh, filter, group_by, order_by, ascending, per_group, offset, limit):
    """infx_engine_list_group_members on session handle sh: a GroupMembersListing for one request (given by its parts), a list of them for a sequence of
    GroupMembersRequest."""
    def pack(r):
        off, lim, per = int(r.offset), int(r.limit), int(r.per_group)
        # out of the C fields' range: passed as values the engine refuses for this request alone
        return _GroupMembersReq(None if r.filter is None else r.filter.encode(), None if r.group_by is None else str(r.group_by).encode(),
                                None if r.order_by is None else r.order_by.encode(), 1 if r.ascending else 0,
                                off if 0 <= off < 2 ** 32 else 0xFFFFFFFF, lim if 0 <= lim < 2 ** 32 else 0, per if 0 <= per < 2 ** 32 else 0)
    texts = _value_texts(engine)

    def read(i, r):
        groups = C.c_uint32(0); tot = C.c_uint32(0)
        engine._check(engine.L.infx_engine_group_members_totals(sh, i, C.byref(groups), C.byref(tot)))
        gcodes = np.zeros(1024, np.uint32); sizes = np.zeros(1024, np.uint32); held = np.zeros(1024, np.uint32)
        keys = np.zeros(4096, np.int64); docs = np.zeros(4096, np.int32); codes = np.zeros(4096, np.uint32)
        m = engine.L.infx_engine_group_members_rows(sh, i, _p(gcodes, C.c_uint32), _p(sizes, C.c_uint32), _p(held, C.c_uint32), 1024)
        k = engine.L.infx_engine_group_members_members(sh, i, _p(keys, C.c_int64), _p(docs, C.c_int32), _p(codes, C.c_uint32), 4096)
        if m < 0 or k < 0 or k != int(held[:m].sum()):
            engine._check(1)
        names = texts(str(r.group_by), gcodes[:m])
        vals = None if r.order_by is None else texts(r.order_by, codes[:k])
        rows, at = [], 0
        for j in range(m):
            h = int(held[j])
            rows.append(GroupMembers(names[j], int(sizes[j]), [int(x) for x in keys[at:at + h]], [] if vals is None else vals[at:at + h]))
            at += h
        return GroupMembersListing(rows, int(groups.value), int(tot.value), None)
    single = filter is None or isinstance(filter, str)
    # (one mask slot per distinct filter: sixteen requests per device call)
    return _per_request(engine, sh, "infx_engine_list_group_members", "infx_engine_group_members_error", _GroupMembersReq,
                        [GroupMembersRequest(filter, group_by, order_by, ascending, per_group, offset, limit)] if single else list(filter), single, pack, read,
                        lambda _, msg: GroupMembersListing(error=msg))


def _edge_arrays(edges, keep):
    """(number of edges, int64 pointer or None, double pointer) of a request's edges; the arrays are appended to keep, which must outlive the call.  Integer
    edges only when every edge is a Python int (not a bool) that an int64 holds; double edges always (what float() refuses is passed as NaN: refused)."""
    ed = tuple(edges)
    ei = None
    if ed and all(isinstance(x, int) and not isinstance(x, bool) and -2 ** 63 <= x < 2 ** 63 for x in ed):
        ei = np.asarray(ed, np.int64); keep.append(ei)
    vals = []
    for x in ed:
        try:
            vals.append(float(x))
        except (TypeError, ValueError, OverflowError):
            vals.append(float("nan"))
    edd = np.asarray(vals, np.float64); keep.append(edd)
    return min(len(ed), 0xFFFFFFFF), None if ei is None else _p(ei, C.c_int64), _p(edd, C.c_double)


def _range_facets(engine, sh, filter, field, edges):
    """infx_engine_range_facets on session handle sh: a RangeFacets for one request (given by its parts), a list of them for a sequence of RangeRequest."""
    keep = []                                            # the edge arrays live until the calls have returned

    def pack(r):
        return _RangeReq(None if r.filter is None else r.filter.encode(), None if r.field is None else str(r.field).encode(), *_edge_arrays(r.edges, keep))

    def read(i, r):
        tot = C.c_uint32(0); below = C.c_uint32(0); above = C.c_uint32(0); nan = C.c_uint32(0)
        engine._check(engine.L.infx_engine_range_total(sh, i, C.byref(tot)))
        counts = np.zeros(256, np.uint32)
        m = engine.L.infx_engine_range_counts(sh, i, _p(counts, C.c_uint32), 256, C.byref(below), C.byref(above), C.byref(nan))
        if m < 0:
            engine._check(1)
        kind = C.c_int32(0); li = C.c_int64(0); hi = C.c_int64(0); ld = C.c_double(0); hd = C.c_double(0)
        engine._check(engine.L.infx_engine_range_minmax(sh, i, C.byref(kind), C.byref(li), C.byref(hi), C.byref(ld), C.byref(hd)))
        lo, up = (int(li.value), int(hi.value)) if kind.value == 1 else ((float(ld.value), float(hd.value)) if kind.value == 2 else (None, None))
        return RangeFacets(tuple(r.edges), [int(c) for c in counts[:m]], int(below.value), int(above.value), int(nan.value), int(tot.value), lo, up, None)
    single = filter is None or isinstance(filter, str)
    # (one mask slot per distinct filter: sixteen requests per device call)
    return _per_request(engine, sh, "infx_engine_range_facets", "infx_engine_range_error", _RangeReq,
                        [RangeRequest(filter, field, edges)] if single else list(filter), single, pack, read,
                        lambda r, msg: RangeFacets(tuple(r.edges), [], 0, 0, 0, 0, None, None, msg))


_STATS_FIGURES = np.dtype([(name, {C.c_uint32: "<u4", C.c_int32: "<i4", C.c_int64: "<i8", C.c_uint64: "<u8", C.c_double: "<f8"}[ty]) for name, ty in _StatsFigures._fields_])


def _stats_figures(f):
    """(count, nan, min, max, sum, mean) of an infx_stats_figures given as the tuple of its fields; the int column's sum is composed here from its two halves."""
    count, nan, kind, _, min_i, max_i, min_d, max_d, sum_d, sum_lo, sum_hi, mean = f
    lo, up = ((min_i, max_i) if kind == 1 else (min_d, max_d)) if count else (None, None)
    return count, nan, lo, up, (sum_hi << 64) + sum_lo if kind == 1 else sum_d, mean if count else None


def _field_stats(engine, sh, filter, field, group_by):
    """infx_engine_field_stats on session handle sh: a FieldStats for one request (given by its parts), a list of them for a sequence of StatsRequest."""
    def pack(r):
        return _StatsReq(*[None if x is None else str(x).encode() for x in (r.filter, r.field, r.group_by)])

    def read(i, r):
        tot = C.c_uint32(0); whole = _StatsFigures()
        engine._check(engine.L.infx_engine_field_stats_total(sh, i, C.byref(tot)))
        engine._check(engine.L.infx_engine_field_stats_whole(sh, i, C.byref(whole)))
        col = C.c_int32(-1)
        m = engine.L.infx_engine_field_stats_groups(sh, i, C.byref(col), None, None, 0)
        if m < 0:
            engine._check(1)
        groups = []
        if m > 0:
            codes = np.zeros(m, np.uint32); figs = (_StatsFigures * m)()
            engine.L.infx_engine_field_stats_groups(sh, i, C.byref(col), _p(codes, C.c_uint32), figs, m)
            vb = C.create_string_buffer(1024)
            for code, f in zip(codes.tolist(), np.frombuffer(figs, _STATS_FIGURES).tolist()):      # (one conversion for all groups: thousands of them are common)
                engine.L.infx_engine_column_value(engine.h, col.value, code, vb, 1024)
                groups.append(GroupStats(vb.value.decode(), *_stats_figures(f)))
        count, nan, lo, up, total, mean = _stats_figures(np.frombuffer(whole, _STATS_FIGURES)[0].tolist())
        return FieldStats(count, nan, int(tot.value), lo, up, total, mean, groups, None)
    single = filter is None or isinstance(filter, str)
    # (one mask slot per distinct filter: sixteen requests per device call)
    return _per_request(engine, sh, "infx_engine_field_stats", "infx_engine_field_stats_error", _StatsReq,
                        [StatsRequest(filter, field, group_by)] if single else list(filter), single, pack, read,
                        lambda r, msg: FieldStats(error=msg))


def _bucket_stats(engine, sh, filter, field, bucket_by, edges):
    """infx_engine_bucket_stats on session handle sh: a BucketStats for one request (given by its parts), a list of them for a sequence of BucketStatsRequest."""
    keep = []                                            # the edge arrays live until the calls have returned

    def pack(r):
        return _BucketStatsReq(*[None if x is None else str(x).encode() for x in (r.filter, r.field, r.bucket_by)], *_edge_arrays(r.edges, keep))

    def row(size, f):
        return BucketRow(size, *_stats_figures(f))

    def read(i, r):
        tot = C.c_uint32(0); whole = _StatsFigures()
        engine._check(engine.L.infx_engine_bucket_stats_total(sh, i, C.byref(tot)))
        engine._check(engine.L.infx_engine_bucket_stats_whole(sh, i, C.byref(whole)))
        m = engine.L.infx_engine_bucket_stats_rows(sh, i, None, None, 0)
        if m < 3:
            engine._check(1)
        sizes = np.zeros(m, np.uint32); figs = (_StatsFigures * m)()
        engine.L.infx_engine_bucket_stats_rows(sh, i, _p(sizes, C.c_uint32), figs, m)
        rows = [row(s, f) for s, f in zip(sizes.tolist(), np.frombuffer(figs, _STATS_FIGURES).tolist())]      # [below | B buckets | above | nan]
        w = np.frombuffer(whole, _STATS_FIGURES)[0].tolist()
        return BucketStats(tuple(r.edges), rows[1:m - 2], rows[0], rows[m - 2], rows[m - 1], row(w[0] + w[1], w), int(tot.value), None)
    single = filter is None or isinstance(filter, str)
    # (one mask slot per distinct filter: sixteen requests per device call)
    return _per_request(engine, sh, "infx_engine_bucket_stats", "infx_engine_bucket_stats_error", _BucketStatsReq,
                        [BucketStatsRequest(filter, field, bucket_by, edges)] if single else list(filter), single, pack, read,
                        lambda r, msg: BucketStats(edges=tuple(r.edges), error=msg))


_DISTINCT_FIGURES = np.dtype([("size", "<u4"), ("distinct", "<u4")])


def _field_distinct(engine, sh, filter, field, group_by):
    """infx_engine_field_distinct on session handle sh: a FieldDistinct for one request (given by its parts), a list of them for a sequence of DistinctRequest."""
    def pack(r):
        return _DistinctReq(*[None if x is None else str(x).encode() for x in (r.filter, r.field, r.group_by)])

    def read(i, r):
        whole = _DistinctFigures()
        engine._check(engine.L.infx_engine_field_distinct_whole(sh, i, C.byref(whole)))
        col = C.c_int32(-1)
        m = engine.L.infx_engine_field_distinct_groups(sh, i, C.byref(col), None, None, 0)
        if m < 0:
            engine._check(1)
        groups = []
        if m > 0:
            codes = np.zeros(m, np.uint32); figs = (_DistinctFigures * m)()
            engine.L.infx_engine_field_distinct_groups(sh, i, C.byref(col), _p(codes, C.c_uint32), figs, m)
            vb = C.create_string_buffer(1024)
            for code, (size, distinct) in zip(codes.tolist(), np.frombuffer(figs, _DISTINCT_FIGURES).tolist()):
                engine.L.infx_engine_column_value(engine.h, col.value, code, vb, 1024)
                groups.append(GroupDistinct(vb.value.decode(), size, distinct))
        return FieldDistinct(int(whole.distinct), int(whole.size), groups, None)
    single = filter is None or isinstance(filter, str)
    # (one mask slot per distinct filter: sixteen requests per device call)
    return _per_request(engine, sh, "infx_engine_field_distinct", "infx_engine_field_distinct_error", _DistinctReq,
                        [DistinctRequest(filter, field, group_by)] if single else list(filter), single, pack, read,
                        lambda r, msg: FieldDistinct(error=msg))


def _top_groups(engine, sh, filter, group_by, by, field, ascending, offset, limit):
    """infx_engine_top_groups on session handle sh: a TopGroups for one request (given by its parts), a list of them for a sequence of TopGroupsRequest."""
    def pack(r):
        off, lim = int(r.offset), int(r.limit)
        # out of the C fields' range: passed as values the engine refuses for this request alone
        return _TopReq(*[None if x is None else str(x).encode() for x in (r.filter, r.group_by, r.by, r.field)], 1 if r.ascending else 0,
                       off if 0 <= off < 2 ** 32 else 0xFFFFFFFF, lim if 0 <= lim < 2 ** 32 else 0)

    def read(i, r):
        groups = C.c_uint32(0); tot = C.c_uint32(0)
        engine._check(engine.L.infx_engine_top_groups_totals(sh, i, C.byref(groups), C.byref(tot)))
        cap = max(1, min(int(r.limit), 1024))                # (an answered request's limit is in range)
        col = C.c_int32(-1); codes = np.zeros(cap, np.uint32); sizes = np.zeros(cap, np.uint32); figs = (_StatsFigures * cap)()
        m = engine.L.infx_engine_top_groups_rows(sh, i, C.byref(col), _p(codes, C.c_uint32), _p(sizes, C.c_uint32), figs, cap)
        if m < 0:
            engine._check(1)
        rows = []
        vb = C.create_string_buffer(1024)
        for code, size, f in zip(codes[:m].tolist(), sizes[:m].tolist(), np.frombuffer(figs, _STATS_FIGURES)[:m].tolist()):
            engine.L.infx_engine_column_value(engine.h, col.value, code, vb, 1024)
            rows.append(GroupRow(vb.value.decode(), size, *(_stats_figures(f) if r.field is not None else ())))
        return TopGroups(rows, int(groups.value), int(tot.value), None)
    single = filter is None or isinstance(filter, str)
    # (one mask slot per distinct filter: sixteen requests per device call)
    return _per_request(engine, sh, "infx_engine_top_groups", "infx_engine_top_groups_error", _TopReq,
                        [TopGroupsRequest(filter, group_by, by, field, ascending, offset, limit)] if single else list(filter), single, pack, read,
                        lambda r, msg: TopGroups(error=msg))


def _quantile_tuple(q):
    """The quantiles of a request as a tuple of floats: a number alone is one quantile; what float() refuses becomes a NaN, which the engine refuses."""
    out = []
    for x in (q if isinstance(q, (tuple, list, np.ndarray)) else (q,)):
        try:
            out.append(float(x))
        except (TypeError, ValueError, OverflowError):
            out.append(float("nan"))
    return tuple(out)


def _quantile_figures(f):
    """(count, nan, values) of an infx_quantile_figures: None for every quantile of a slot without a non-NaN member."""
    nq, count = int(f.nq), int(f.count)
    vals = [None] * nq if not count else ([int(f.v_i[t]) for t in range(nq)] if f.kind == 1 else [float(f.v_d[t]) for t in range(nq)])
    return count, int(f.nan), vals


def _field_quantiles(engine, sh, filter, field, q, group_by):
    """infx_engine_field_quantiles on session handle sh: a FieldQuantiles for one request (given by its parts), a list of them for a sequence of QuantileRequest."""
    keep = []                                            # the quantile arrays live until the calls have returned

    def pack(r):
        qs = np.asarray(_quantile_tuple(r.q), np.float64); keep.append(qs)
        text = [None if x is None else str(x).encode() for x in (r.filter, r.field, r.group_by)]
        return _QuantReq(text[0], text[1], text[2], _p(qs, C.c_double) if len(qs) else None, min(len(qs), 0xFFFFFFFF))

    def read(i, r):
        tot = C.c_uint32(0); whole = _QuantFigures()
        engine._check(engine.L.infx_engine_field_quantiles_total(sh, i, C.byref(tot)))
        engine._check(engine.L.infx_engine_field_quantiles_whole(sh, i, C.byref(whole)))
        col = C.c_int32(-1)
        m = engine.L.infx_engine_field_quantiles_groups(sh, i, C.byref(col), None, None, 0)
        if m < 0:
            engine._check(1)
        groups = []
        if m > 0:
            codes = np.zeros(m, np.uint32); figs = (_QuantFigures * m)()
            engine.L.infx_engine_field_quantiles_groups(sh, i, C.byref(col), _p(codes, C.c_uint32), figs, m)
            vb = C.create_string_buffer(1024)
            for code, f in zip(codes.tolist(), figs):
                engine.L.infx_engine_column_value(engine.h, col.value, code, vb, 1024)
                groups.append(GroupQuantiles(vb.value.decode(), *_quantile_figures(f)))
        count, nan, vals = _quantile_figures(whole)
        return FieldQuantiles(_quantile_tuple(r.q), vals, count, nan, int(tot.value), groups, None)
    single = filter is None or isinstance(filter, str)
    # (one mask slot per distinct filter: sixteen requests per device call)
    return _per_request(engine, sh, "infx_engine_field_quantiles", "infx_engine_field_quantiles_error", _QuantReq,
                        [QuantileRequest(filter, field, q, group_by)] if single else list(filter), single, pack, read,
                        lambda r, msg: FieldQuantiles(q=_quantile_tuple(r.q), error=msg))


def _attach_pre_filter_facets(engine, sh, qs, results):
    """Query.pre_filter_facets of a batch just searched on session handle sh: the distinct pre-filters that ran are counted in ONE facets_of_documents call
    (a device batch carries at most 16, so at most one pass; none when the engine has them cached) and each asking query gets its expression's facets."""
    want = []
    for q, r in zip(qs, results):
        if q.pre_filter_facets and q.pre_filter is not None and r.error is None and q.pre_filter not in want:
            want.append(q.pre_filter)
    if not want:
        return
    got = dict(zip(want, _facets_filtered(engine, sh, want)))
    for q, r in zip(qs, results):
        if q.pre_filter_facets and q.pre_filter is not None and r.error is None and got[q.pre_filter].error is None:
            r.pre_filter_facets = got[q.pre_filter].facets


def _set_sort(engine, sh, sort_by, ascending):
    engine._check(engine.L.infx_engine_set_sort(sh, sort_by.encode() if sort_by is not None else None, int(bool(ascending))))


def normalize(s, lower=False):
    L = load_library()
    x = _u16(s); out = np.zeros(len(x) + 8, np.uint16)
    n = L.infx_engine_normalize(_p(x, C.c_uint16), len(x), int(lower), _p(out, C.c_uint16), len(out))
    return out[:n].tobytes().decode("utf-16-le", errors="surrogatepass")
