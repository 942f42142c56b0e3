// List columns, host side: a document field that holds a LIST of values (Field.IsArray: a film's genres, a product's tags) in filters and facets.
//
// Reference: Api/Field.cs (IsArray carries a List<object>); Core/FacetBuilder.cs:82-91, 143-152 counts every element of such a field.
//
// Storage: the elements of all documents, in document order (order and duplicates kept), are dictionary-encoded with encode_column's rules — the same Boxed
// dictionary, text and rank a scalar column has — and the documents' lists are a CSR pair over the codes: off[n + 1] and dict.codes[total].
//
// Filters: a leaf over a list column holds for a document iff its list is non-empty and leaf_holds() is true for at least one element, or its list is
// empty and leaf_holds() is true for a null value (so `tags IS NULL` accepts the empty lists, as do `<` and `<=`, which order a null below every constant; no other comparison does).  NOT / AND / OR / ?: apply to that
// verdict as to any other: `NOT tags = 'sale'` — and `tags != 'sale'`, which the parser lowers to NOT over an EQ leaf — mean "no element equals sale".
// The engine lowers such a leaf to a DERIVED one-bit scalar column (k_list_leaf, csrc/list_columns.hip.inc): the leaf's bitmap over the element dictionary
// (leaf_table) plus the empty-list bit give 0 or 1 per document, and the program gets an ordinary leaf over that column with num_values = 2 and a table in
// which only bit 1 is set.  What is here is that arithmetic, shared by the engine and by tests/models/list_columns_model.cpp.
#pragma once
#include "filter.h"

namespace infx { namespace filt {

struct ListColumn {
    std::string name; bool facetable = false; int32_t kind = 0;      // name "": a free slot.  kind: 1 int64, 2 double, 3 string (0: no element anywhere)
    Column dict;                    // the element dictionary; dict.codes = the element codes of all documents in document order
    std::vector<uint32_t> off;      // n + 1: document d's elements are dict.codes[off[d] .. off[d + 1])
    bool live() const { return !name.empty(); }
    size_t docs() const { return off.empty() ? 0 : off.size() - 1; }
};

// the leaf's bitmap over the element codes; returns the leaf's verdict on an empty list (= on a null value)
inline bool list_leaf_table(const Leaf& L, const ListColumn& c, std::vector<uint32_t>& words) {
    leaf_table(L, &c.dict, words);
    return leaf_holds(L, Boxed());
}
// the derived bit of document d, as k_list_leaf computes it
inline bool list_leaf_bit(const ListColumn& c, const std::vector<uint32_t>& words, bool emptyBit, size_t d) {
    if (c.off[d] == c.off[d + 1]) return emptyBit;
    for (uint32_t e = c.off[d]; e < c.off[d + 1]; e++) { const uint32_t v = c.dict.codes[e]; if ((words[v >> 5] >> (v & 31)) & 1u) return true; }
    return false;
}
// k bitmaps of W words each side by side, word w of leaf i at maps[w * k + i]: one element code reads k consecutive words
inline void list_leaf_maps(const std::vector<std::vector<uint32_t>>& tables, size_t W, std::vector<uint32_t>& maps) {
    const size_t k = tables.size();
    maps.assign(W * k, 0u);
    for (size_t i = 0; i < k; i++) for (size_t w = 0; w < W && w < tables[i].size(); w++) maps[w * k + i] = tables[i][w];
}
// what identifies a leaf's derived column within its list column: the operator and the constants (length-prefixed: no two leaves share a key)
inline std::string list_leaf_key(const Leaf& L) {
    std::string k = std::to_string((int)L.op);
    for (auto& c : L.consts) { k += ':'; k += std::to_string(c.size()); k += ':'; k += c; }
    return k;
}

}} // namespace
