// Test shim: the oracle's C ABI (oracle/oracle_c.cpp, included as it stands) plus ONE setter for the CoverageSetup its coverage engine and pipeline read
// (oracle/coverage.hpp:19-26).  Built at test time by tests/oracle_setup.py; the oracle itself has no setter.
#include "../../oracle/oracle_c.cpp"

// v: MinWordSize, LevenshteinMaxWordSize, NumTypos, MinLengthOneTypo, MinLengthTwoTypos, CoverageMinWordHitsAbs, CoverageMinWordHitsRelative,
//    CoverageQLimitForErrorTolerance, CoverWholeQuery, CoverWholeWords, CoverFuzzyWords, CoverJoinedWords, CoverPrefixSuffix, Truncate, TruncationScore
extern "C" void orc_set_coverage_setup(void* h, const int32_t* v, double relativeq) {
    orc::CoverageSetup& s = ((Handle*)h)->eng.cov.setup;
    s.MinWordSize = v[0]; s.LevenshteinMaxWordSize = v[1]; s.NumTypos = v[2]; s.MinLengthOneTypo = v[3]; s.MinLengthTwoTypos = v[4];
    s.CoverageMinWordHitsAbs = v[5]; s.CoverageMinWordHitsRelative = v[6]; s.CoverageQLimitForErrorTolerance = v[7];
    s.CoverageLcsErrorToleranceRelativeq = relativeq;
    s.CoverWholeQuery = v[8] != 0; s.CoverWholeWords = v[9] != 0; s.CoverFuzzyWords = v[10] != 0; s.CoverJoinedWords = v[11] != 0; s.CoverPrefixSuffix = v[12] != 0;
    s.Truncate = v[13] != 0; s.TruncationScore = (uint8_t)v[14];
}
