"""The Python Query / Boost / BoostStrength surface against the reference's Api/Query.cs, Api/Boost.cs and Api/BoostStrength.cs (no GPU needed)."""
import inspect

from infidex_amd import Query, Boost, BoostStrength, SearchEngine, Session
from infidex_amd import sharded


def test_boost_strength_values():
    assert (BoostStrength.Low, BoostStrength.Med, BoostStrength.High) == (1, 2, 3)


def test_query_defaults_follow_the_reference():
    q = Query("alpha")
    assert q.max_number_of_records_to_return == 10 and q.coverage_depth == 500 and q.enable_coverage is True
    assert q.filter is None and q.enable_facets is False
    assert q.enable_boost is False and q.boosts is None                  # EnableBoost defaults to false, Boosts to null
    assert q.sort_by is None and q.sort_ascending is False               # SortBy null = relevance; SortAscending false
    assert q.max_boost == 0


def test_max_boost():
    bs = [Boost("a = 1", BoostStrength.High), Boost(None, BoostStrength.Med), Boost("b = 2", BoostStrength.Low)]
    assert Query("x", boosts=bs).max_boost == 0                          # EnableBoost off
    assert Query("x", enable_boost=True).max_boost == 0                  # Boosts null
    assert Query("x", enable_boost=True, boosts=bs).max_boost == 6       # every boost counts, the null-filter one included
    assert Boost("a = 1").strength == BoostStrength.Med


def test_new_arguments_default_to_the_old_behaviour():
    for fn in (SearchEngine.search_filtered,):
        p = inspect.signature(fn).parameters
        assert p["enable_boost"].default is False and p["boosts"].default is None
        assert p["sort_by"].default is None and p["sort_ascending"].default is False
    assert hasattr(Session, "set_boosts") and hasattr(Session, "set_sort")
    for name in ("set_boosts", "set_sort"):
        assert hasattr(sharded.ShardSession, name) and hasattr(sharded.ShardedSearcher, name)
    assert callable(sharded.simulate_set_boosts) and callable(sharded.simulate_set_sort)
