"""infidex_amd — MI355X-native drop-in for the query-time scoring hot path of lofcz/Infidex.

Python is plumbing only (ctypes over libinfidex_hip.so); the product is the HIP kernels + the C ABI
(include/infidex_hip.h) + the C++ host engine (include/infidex_engine.h). There is no CPU scoring path:
Search raises if the HIP extension or a GPU is missing.
"""
from .engine import (SearchEngine, Session, Query, CoverageSetup, Boost, BoostStrength, Document, Field, Weight, Result, ScoreEntry, InfidexError,
                     FilteredFacets, Listing, ListRequest, GroupListing, GroupListRequest, GroupMembersListing, GroupMembers, GroupMembersRequest, RangeFacets, RangeRequest, FieldStats, GroupStats, StatsRequest, BucketStats, BucketRow, BucketStatsRequest, FieldQuantiles, GroupQuantiles, QuantileRequest, TopGroups, GroupRow, TopGroupsRequest, FieldDistinct, GroupDistinct, DistinctRequest, Highlight, TermMatch, load_library, LIB_PATH, MAX_PREFILTERS)

__all__ = ["SearchEngine", "Session", "Query", "CoverageSetup", "Boost", "BoostStrength", "Document", "Field", "Weight", "Result", "ScoreEntry", "InfidexError",
           "FilteredFacets", "Listing", "ListRequest", "GroupListing", "GroupListRequest", "GroupMembersListing", "GroupMembers", "GroupMembersRequest", "RangeFacets", "RangeRequest", "FieldStats", "GroupStats", "StatsRequest", "BucketStats", "BucketRow", "BucketStatsRequest", "FieldQuantiles", "GroupQuantiles", "QuantileRequest", "TopGroups", "GroupRow", "TopGroupsRequest", "FieldDistinct", "GroupDistinct", "DistinctRequest", "Highlight", "TermMatch", "load_library", "LIB_PATH", "MAX_PREFILTERS"]
