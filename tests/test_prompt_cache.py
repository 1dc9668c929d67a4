"""PromptCache / PrefixSharing (llama-gguf_amd/hip_backend.py) against the reference's src/model/cache.rs: its four known-answer
tests (cache.rs:352-428) and each behaviour the restatement keeps as written.  CPU only: a fake engine hands out handles that record
free(), so that every evicted, removed and cleared entry can be checked to release its device memory exactly once."""
import pytest


class Handle:
    def __init__(self, nbytes, log):
        self.nbytes, self.freed, self._log = nbytes, 0, log

    def free(self):
        self.freed += 1
        self._log.append(self)


class Engine:
    """prefix_save / prefix_restore as HipGpuInference has them; 64 bytes per row."""

    def __init__(self):
        self.freed, self.saved, self.restored = [], [], []

    def prefix_save(self, n=None, slot=-1):
        h = Handle(64 * n, self.freed)
        self.saved.append((h, n, slot))
        return h

    def prefix_restore(self, prefix, slot=-1, n=None):
        self.restored.append((prefix, slot, n))


@pytest.fixture
def hb(pkg):
    return pkg.hip_backend


def _cache(hb, **kw):
    return hb.PromptCache(hb.PromptCacheConfig(**kw))


def test_default_config_is_the_references(hb):
    c = hb.PromptCacheConfig()
    assert (c.max_entries, c.max_memory, c.min_prefix_len, c.cache_system_prompts) == (100, 1024 * 1024 * 1024, 32, True)


# ---- cache.rs:352-428 ----
def test_prefix_id(hb):
    assert hb.prefix_id([1, 2, 3, 4]) == hb.prefix_id([1, 2, 3, 4])
    assert hb.prefix_id([1, 2, 3, 4]) != hb.prefix_id([1, 2, 3, 5])
    assert 0 <= hb.prefix_id([1, 2, 3, 4]) < 2 ** 64
    assert hb.prefix_id([1, 2]) != hb.prefix_id([1, 2, 0])


def test_prompt_cache(hb):
    cache = _cache(hb, min_prefix_len=2)
    pid = cache.cache_prefix([1, 2, 3, 4, 5], Handle(128, []))
    assert cache.get_prefix(pid) is not None
    assert cache.stats().num_entries == 1


def test_find_matching_prefix(hb):
    cache = _cache(hb, min_prefix_len=2)
    cache.cache_prefix([1, 2, 3], Handle(128, []))
    result = cache.find_matching_prefix([1, 2, 3, 4, 5])
    assert result is not None and result[1] == 3
    assert cache.find_matching_prefix([1, 2, 4, 5]) is None


def test_cache_eviction(hb):
    cache = _cache(hb, max_entries=2, min_prefix_len=1)
    for i in range(3):
        cache.cache_prefix([i], Handle(128, []))
    assert cache.stats().num_entries <= 2


# ---- the behaviours kept as written ----
def test_known_id_bumps_the_count_refreshes_the_stamp_and_stores_nothing(hb):
    log = []
    cache = _cache(hb, min_prefix_len=1)
    first, other, second = Handle(100, log), Handle(100, log), Handle(100, log)
    pid = cache.cache_prefix([7, 8], first)
    cache.cache_prefix([9], other)
    e = cache.entries[pid]
    stamp, used = e.last_access, cache.memory_used
    assert e.ref_count == 0 and e.last_access < cache.entries[hb.prefix_id([9])].last_access
    assert cache.cache_prefix([7, 8], second) == pid
    assert e.handle is first and e.ref_count == 1 and e.last_access > cache.entries[hb.prefix_id([9])].last_access > stamp
    assert cache.memory_used == used and cache.stats().num_entries == 2
    assert (first.freed, second.freed) == (0, 1)          # the caller's new handle is released, the stored one kept


def test_short_prompt_returns_its_id_and_is_not_stored(hb):
    log = []
    cache = _cache(hb, min_prefix_len=4)
    h = Handle(100, log)
    assert cache.cache_prefix([1, 2, 3], h) == hb.prefix_id([1, 2, 3])
    assert cache.stats().num_entries == 0 and cache.memory_used == 0 and h.freed == 1
    assert cache.get_prefix(hb.prefix_id([1, 2, 3])) is None


def test_memory_size_is_device_bytes_plus_four_per_token(hb):
    cache = _cache(hb, min_prefix_len=1)
    cache.cache_prefix([1, 2, 3], Handle(1000, []))
    cache.cache_prefix([4, 5], Handle(50, []))
    s = cache.stats()
    assert (s.num_entries, s.memory_used, s.total_tokens_cached) == (2, 1000 + 12 + 50 + 8, 5)


def test_eviction_under_max_entries_takes_the_least_recently_used_idle_entry(hb):
    log = []
    cache = _cache(hb, max_entries=2, min_prefix_len=1)
    a, b, c = Handle(10, log), Handle(10, log), Handle(10, log)
    ia, ib = cache.cache_prefix([1], a), cache.cache_prefix([2], b)
    cache.get_prefix(ia)                                   # a: newer stamp, but now referenced
    cache.release_prefix(ia)                               # ... and idle again: b is the older idle entry
    ic = cache.cache_prefix([3], c)
    assert set(cache.entries) == {ia, ic}
    assert (a.freed, b.freed, c.freed) == (0, 1, 0) and log == [b]
    assert cache.memory_used == 2 * 14


def test_eviction_under_max_memory_evicts_until_the_entry_fits(hb):
    log = []
    cache = _cache(hb, max_memory=100, min_prefix_len=1)
    hs = [Handle(36, log) for _ in range(3)]               # 40 bytes each with the token
    ids = [cache.cache_prefix([i], h) for i, h in enumerate(hs)]
    assert set(cache.entries) == {ids[1], ids[2]} and log == [hs[0]] and cache.memory_used == 80
    big = Handle(90, log)                                  # 94: both others must go
    ib = cache.cache_prefix([9], big)
    assert set(cache.entries) == {ib} and log == [hs[0], hs[1], hs[2]] and cache.memory_used == 94
    assert all(h.freed == 1 for h in hs) and big.freed == 0


def test_eviction_stops_at_referenced_entries_and_inserts_anyway(hb):
    log = []
    cache = _cache(hb, max_entries=2, min_prefix_len=1)
    ia, ib = cache.cache_prefix([1], Handle(10, log)), cache.cache_prefix([2], Handle(10, log))
    cache.get_prefix(ia)
    cache.get_prefix(ib)
    ic = cache.cache_prefix([3], Handle(10, log))
    assert set(cache.entries) == {ia, ib, ic} and log == []          # over max_entries: nothing idle to evict
    assert cache.stats().num_entries == 3


def test_find_takes_the_longest_match_and_bumps_only_it(hb):
    cache = _cache(hb, min_prefix_len=1)
    i2, i3, ix = cache.cache_prefix([1, 2], Handle(1, [])), cache.cache_prefix([1, 2, 3], Handle(1, [])), cache.cache_prefix([1, 9], Handle(1, []))
    assert cache.find_matching_prefix([1, 2, 3, 4]) == (i3, 3)
    assert [cache.entries[i].ref_count for i in (i2, i3, ix)] == [0, 1, 0]
    assert cache.find_matching_prefix([1, 2]) == (i2, 2)              # a query as long as the entry matches
    assert cache.find_matching_prefix([1]) is None                    # shorter than every entry
    assert cache.entries[i3].last_access < cache.entries[i2].last_access


def test_try_restore_bumps_twice_and_release_active_drops_once(hb):
    eng = Engine()
    ps = hb.PrefixSharing(hb.PromptCacheConfig(min_prefix_len=2))
    assert ps.try_restore([1, 2, 3], eng) == 0 and eng.restored == []
    pid = ps.save_prefix([1, 2, 3], eng, slot=2)
    assert eng.saved[0][1:] == (3, 2) and ps.active_prefix == pid
    e = ps.cache.entries[pid]
    assert e.ref_count == 0
    ps.release_active()
    assert ps.active_prefix is None and e.ref_count == 0              # saturating
    assert ps.try_restore([1, 2, 3, 4, 5], eng, slot=1) == 3
    assert eng.restored == [(e.handle, 1, 3)]
    assert e.ref_count == 2 and ps.active_prefix == pid
    ps.release_active()
    assert e.ref_count == 1 and ps.active_prefix is None
    ps.release_active()                                               # no active prefix: nothing happens
    assert e.ref_count == 1
    assert ps.stats().num_entries == 1 and ps.stats().memory_used == 64 * 3 + 12


def test_saving_a_known_prompt_again_frees_the_new_copy(hb):
    eng = Engine()
    ps = hb.PrefixSharing(hb.PromptCacheConfig(min_prefix_len=2))
    pid = ps.save_prefix([4, 5, 6], eng)
    assert ps.save_prefix([4, 5, 6], eng) == pid
    assert [h.freed for h, _, _ in eng.saved] == [0, 1]
    assert ps.cache.entries[pid].ref_count == 1 and ps.stats().num_entries == 1


def test_removed_and_cleared_handles_are_freed_exactly_once(hb):
    eng = Engine()
    ps = hb.PrefixSharing(hb.PromptCacheConfig(min_prefix_len=1, max_entries=3))
    ids = [ps.save_prefix([i, i], eng) for i in range(4)]              # the fourth evicts the first
    handles = [h for h, _, _ in eng.saved]
    assert [h.freed for h in handles] == [1, 0, 0, 0]
    ps.cache.remove_prefix(ids[1])
    ps.cache.remove_prefix(ids[1])                                    # a second removal finds nothing
    assert [h.freed for h in handles] == [1, 1, 0, 0]
    assert ps.stats().memory_used == 2 * (128 + 8)
    ps.clear()
    assert [h.freed for h in handles] == [1, 1, 1, 1] and len(eng.freed) == 4
    assert ps.active_prefix is None and ps.stats().num_entries == 0 and ps.stats().memory_used == 0
    ps.clear()
    assert len(eng.freed) == 4
