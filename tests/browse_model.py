"""Test-side model of SearchEngine.HandleEmptyQueryWithFacets (SearchEngine.cs:321-346) and FacetBuilder.BuildFacetsFromAllDocuments
(Core/FacetBuilder.cs:110-181).  Nothing here asks the product: the filter decisions come from the oracle's filter VM (tests.oracle_lib.filter_eval),
the rest is a walk over the documents and plain counting.

Facet order: count descending, then value ascending as the oracle restates `ThenBy(kvp => kvp.Key)` (oracle/filter.hpp: ordinal-ignore-case, then
ordinal).  order_facets folds with str.lower(), the engine and the oracle with the invariant upper-case table: the two orders differ where a value lies
between a letter's lower-case and upper-case form ('_' against 'a'; tests/filter_fuzz.py FOLD_ORDER).  The corpora that go through order_facets have no
such pair — tests/test_filter_model.py::test_order_facets_agrees_on_the_fuzz_corpus holds that for the string column of filter_fuzz.columns — so
str.lower() stays; the engine's own order on such pairs is pinned by test_facet_and_sort_order_follow_the_folding and, on the GPU, by
tests/test_gpu_filter_fuzz.py::test_facet_tie_order_and_sort_by_follow_the_folding."""
import math

import numpy as np

from tests import oracle_lib as O

BROWSE_SCORE_BITS = int(np.float32(65535.0).view(np.uint32))     # ushort.MaxValue as fp32


def facet_text(v):
    """Field.Value.ToString() of a column value (doubles as the oracle prints them); None for null."""
    if v is None:
        return None
    if isinstance(v, (float, np.floating)):
        return O.double_to_string(float(v))
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    return str(v)


def order_facets(counts, limit=100):
    items = [(k, c) for k, c in counts.items() if c > 0]
    items.sort(key=lambda kc: (-kc[1], kc[0].lower(), kc[0]))
    return items[:limit]


class BrowseModel:
    """columns: {name: (values per document, facetable)} in the engine's column order; keys: DocumentKey per document (None: the document index)."""

    def __init__(self, columns, keys=None):
        self.columns = columns
        self.n = len(next(iter(columns.values()))[0])
        self.keys = list(range(self.n)) if keys is None else [int(k) for k in keys]
        self.deleted = set()
        self._memo = {}

    def fields(self, d, names):
        out = {}
        for name in names:
            v = self.columns[name][0][d]
            out[name] = int(v) if isinstance(v, (int, np.integer)) else float(v) if isinstance(v, (float, np.floating)) else v
        return out

    def holds(self, expr, d):
        names = [n for n in self.columns if n in expr]             # the fields the expression can read (a field it does not name cannot matter)
        f = self.fields(d, names)
        k = (expr,) + tuple((v if not (isinstance(v, float) and math.isnan(v)) else "NaN", math.copysign(1.0, v) if isinstance(v, float) and v == 0 else 0)
                            for v in f.values())
        if k not in self._memo:
            self._memo[k] = O.filter_eval(expr, f)
        return self._memo[k]

    def first_live_of_key(self):
        first = {}
        for d in range(self.n):
            if d not in self.deleted:
                first.setdefault(self.keys[d], d)
        return first

    def rows(self, expr, n):
        """The first n live documents, in order, whose key's first live document passes expr (ResultProcessor.ApplyFilter looks rows up by key)."""
        unique = len(set(self.keys)) == self.n
        first = None if unique else self.first_live_of_key()
        out = []
        for d in range(self.n):
            if len(out) >= n:
                break
            if d in self.deleted:
                continue
            rep = d if unique else first[self.keys[d]]
            if expr is None or self.holds(expr, rep):
                out.append(d)
        return out

    def count(self, expr):
        """Filter.NumberOfDocumentsInFilter: every live document's own fields (ResultProcessor.cs:39-54)."""
        return sum(1 for d in range(self.n) if d not in self.deleted and self.holds(expr, d))

    def row_facets(self, docs):
        """FacetBuilder.BuildFacets over rows: each row's document is looked up by key (the key's first live document)."""
        if not docs:
            return {}
        unique = len(set(self.keys)) == self.n
        first = None if unique else self.first_live_of_key()
        out = {}
        for name, (vals, facetable) in self.columns.items():
            if not facetable:
                continue
            c = {}
            for d in docs:
                t = facet_text(vals[d if unique else first[self.keys[d]]])
                if t:
                    c[t] = c.get(t, 0) + 1
            if c:
                out[name] = order_facets(c)
        return out

    def all_facets(self):
        """FacetBuilder.BuildFacetsFromAllDocuments: every live document, per document."""
        out = {}
        for name, (vals, facetable) in self.columns.items():
            if not facetable:
                continue
            c = {}
            for d in range(self.n):
                if d in self.deleted:
                    continue
                t = facet_text(vals[d])
                if t:
                    c[t] = c.get(t, 0) + 1
            if c:
                out[name] = order_facets(c)
        return out

    def check(self, result, expr, n, ctx=None):
        """result (infidex_amd Result) is the browse answer for (expr, n): keys, order, score bits, tiebreakers, facets, flags."""
        docs = self.rows(expr, n)
        assert result.error is None, (ctx, result.error)
        assert [x.document_id for x in result.records] == [self.keys[d] for d in docs], (ctx, [x.document_id for x in result.records][:8], [self.keys[d] for d in docs][:8])
        bits = np.asarray([x.score for x in result.records], np.float32).view(np.uint32)
        assert all(int(b) == BROWSE_SCORE_BITS for b in bits), (ctx, bits)
        assert all(x.tiebreaker == 0 for x in result.records), ctx
        assert (result.facets or {}) == self.row_facets(docs), (ctx, result.facets, self.row_facets(docs))
        assert (result.unsupported, result.used_coverage, result.stage1_fallback, result.skipped_candidates) == (False, False, False, False), ctx
        return docs
