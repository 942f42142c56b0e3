// Host model of the Infiscript filter path: infidex_amd/csrc/host/filter.h UNCHANGED (parser, coercions, dictionary encoding, leaf tables) compiled for the
// host, plus what the device does with its output — a postfix loop over the leaf bitmaps, indexed by each document's codes (filt_eval_codes of
// infidex_amd/csrc/filter.hip.inc, restated here in ten lines).  Test infrastructure (tests/test_filter_model.py); nothing here needs a GPU.
//
//   filter_model fold        prints fold_unit(c) for every c in 0..65535 (hex, one line)
//   filter_model fmt         stdin: one double per line as 16 hex digits of its bits; prints fmt_double of each, one per line
//   filter_model rank        stdin: "<n>", then n string values (UTF-8 in hex, "-" for the empty string); prints the facet tie order rank of each value
//                            (encode_column's Column::rank) on one line and its dense sort rank (sort_rank) on the next
//   filter_model eval        stdin: "<ncols> <ndocs>", then per column "<name> <kind>" (1 int64, 2 double, 3 string) and ndocs value lines (decimal / 16 hex
//                            digits of the bits / the UTF-8 bytes in hex, "-" for the empty string), then "<nexpr>" and one expression per line (UTF-8 in hex).
//                            Prints per expression "OK <ops> <depth> <0/1 per document>" or "ERR <message>"; after them "DICT <name> <distinct values>" per column.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include "../../infidex_amd/csrc/host/filter.h"

using namespace infx::filt;

static std::string unhex(const std::string& h) {
    std::string o; if (h == "-") return o;
    for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
    return o;
}
static double bits_double(const std::string& h) { const uint64_t b = std::stoull(h, nullptr, 16); double d; std::memcpy(&d, &b, 8); return d; }

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "fold") { for (int c = 0; c < 65536; c++) printf("%x ", (unsigned)fold_unit((uint16_t)c)); printf("\n"); return 0; }
    if (mode == "fmt") { std::string h; while (std::cin >> h) printf("%s\n", fmt_double(bits_double(h)).c_str()); return 0; }
    if (mode == "rank") {
        size_t n; std::cin >> n; std::vector<Boxed> v(n);
        for (Boxed& b : v) { std::string t; std::cin >> t; b.kind = 3; b.s = unhex(t); }
        Column c; encode_column(c, n, [&](size_t d) { return v[d]; }, std::string());
        std::vector<uint32_t> sr; sort_rank(c, sr);
        for (size_t d = 0; d < n; d++) printf("%u ", c.rank[c.codes[d]]); printf("\n");
        for (size_t d = 0; d < n; d++) printf("%u ", sr[c.codes[d]]); printf("\n");
        return 0;
    }
    if (mode != "eval") return 2;
    size_t ncols, ndocs, nexpr; std::cin >> ncols >> ndocs;
    std::vector<Column> cols(ncols);
    for (Column& c : cols) {
        int kind; std::cin >> c.name >> kind;
        std::vector<Boxed> v(ndocs);
        for (Boxed& b : v) { std::string t; std::cin >> t; b.kind = kind; if (kind == 1) b.i = std::stoll(t); else if (kind == 2) b.d = bits_double(t); else b.s = unhex(t); }
        if (kind == 1) encode_column(c, ndocs, [&](size_t d) { return v[d]; }, (long long)0);
        else if (kind == 2) encode_column(c, ndocs, [&](size_t d) { return v[d]; }, (uint64_t)0);
        else encode_column(c, ndocs, [&](size_t d) { return v[d]; }, std::string());
    }
    std::cin >> nexpr;
    for (size_t x = 0; x < nexpr; x++) {
        std::string h; std::cin >> h;
        Program P;
        try { P = parse(unhex(h)); } catch (const std::exception& e) { printf("ERR %s\n", e.what()); continue; }
        struct Tab { const Column* col; std::vector<uint32_t> words; };
        std::vector<Tab> tabs(P.leaves.size());
        for (size_t l = 0; l < P.leaves.size(); l++) {
            tabs[l].col = nullptr; for (const Column& c : cols) if (c.name == P.leaves[l].field) tabs[l].col = &c;
            leaf_table(P.leaves[l], tabs[l].col, tabs[l].words);
        }
        std::string out(ndocs, '0'); size_t depth = 0;
        for (size_t d = 0; d < ndocs; d++) {
            std::vector<int> st;                                        // 0 F, 1 T, 2 N (not a bool)
            for (const PIns& in : P.code) {
                if (in.op == P_LEAF) { const Tab& t = tabs[in.arg]; const uint32_t c = t.col ? t.col->codes[d] : 0u; st.push_back((t.words[c >> 5] >> (c & 31)) & 1u); }
                else if (in.op == P_LIT) st.push_back(2);
                else if (in.op == P_NOT) st.back() = st.back() == 1 ? 0 : 1;
                else if (in.op == P_TERN) { const int b = st.back(); st.pop_back(); const int a = st.back(); st.pop_back(); st.back() = st.back() == 0 ? b : a; }
                else { const int r = st.back(); st.pop_back(); const int l = st.back(); st.back() = in.op == P_AND ? (l == 0 ? 0 : r) : (l == 1 ? 1 : r); }
                depth = std::max(depth, st.size());
            }
            if (st.size() == 1 && st[0] == 1) out[d] = '1';
        }
        printf("OK %zu %zu %s\n", P.code.size(), depth, out.c_str());
    }
    for (const Column& c : cols) printf("DICT %s %zu\n", c.name.c_str(), c.dict.size());
    return 0;
}
