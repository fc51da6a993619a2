"""heal_amd/derived.py: the one store of weight-derived tensors (CPU tensors; the capture state is patched)."""
import weakref

import pytest
import torch

from heal_amd import derived


@pytest.fixture
def store(monkeypatch):
    """An empty store and retired list for the test, the real ones restored afterwards; not capturing unless a test says so."""
    monkeypatch.setattr(derived, "_STORE", type(derived._STORE)())
    monkeypatch.setattr(derived, "RETIRED", [])
    monkeypatch.setattr(derived, "capturing", lambda: False)
    return derived


def _double(w, calls):
    def build():
        calls.append(1)
        return w * 2
    return build


def test_hit_on_the_same_versions(store):
    w, calls = torch.arange(4.0), []
    a = store.derived("t", (w,), _double(w, calls))
    b = store.derived("t", (w,), _double(w, calls))
    assert a is b and len(calls) == 1 and store.ready("t", (w,))
    assert not store.ready("t", (w,), extra=(1,)) and not store.ready("other", (w,))


def test_rebuild_after_an_in_place_update(store):
    w, calls = torch.arange(4.0), []
    a = store.derived("t", (w,), _double(w, calls))
    w.mul_(3)
    assert not store.ready("t", (w,))
    b = store.derived("t", (w,), _double(w, calls))
    assert len(calls) == 2 and b is not a and torch.equal(b, torch.arange(4.0) * 6)


def test_none_sources_and_extra_are_part_of_the_slot(store):
    w, calls = torch.ones(3), []
    store.derived("t", (w, None), _double(w, calls))
    store.derived("t", (w, None), _double(w, calls), extra=(True,))
    store.derived("t", (w, None), _double(w, calls))
    assert len(calls) == 2 and store.live() == 2


def test_one_entry_per_slot_and_nothing_retired_while_unpinned(store):
    w, calls = torch.ones(8), []
    for _ in range(100):
        w.add_(1)
        store.derived("t", (w,), _double(w, calls))
    assert len(calls) == 100 and store.live() == 1 and store.RETIRED == []


def test_values_handed_out_while_capturing_are_retired_on_replacement(store, monkeypatch):
    w, calls = torch.ones(8), []
    eager = store.derived("t", (w,), _double(w, calls))
    monkeypatch.setattr(store, "capturing", lambda: True)
    assert store.derived("t", (w,), _double(w, calls)) is eager        # a hit during a capture pins the entry
    monkeypatch.setattr(store, "capturing", lambda: False)
    w.add_(1)
    store.derived("t", (w,), _double(w, calls))
    assert len(calls) == 2 and len(store.RETIRED) == 1 and store.RETIRED[0] is eager


def test_a_value_built_while_capturing_is_not_served_afterwards(store, monkeypatch):
    w, calls = torch.ones(8), []
    monkeypatch.setattr(store, "capturing", lambda: True)
    recorded = store.derived("t", (w,), _double(w, calls))
    assert store.RETIRED == [recorded] and not store.ready("t", (w,)) and store.live() == 0
    monkeypatch.setattr(store, "capturing", lambda: False)
    again = store.derived("t", (w,), _double(w, calls))
    assert again is not recorded and len(calls) == 2 and store.ready("t", (w,))


def test_a_cached_source_is_kept_alive(store):
    p = torch.nn.Parameter(torch.ones(16))
    ref = weakref.ref(p)
    store.derived("t", (p,), lambda: p.detach() * 2)
    del p
    assert ref() is not None
    store._STORE.clear()
    assert ref() is None


def test_the_lru_bound_holds(store, monkeypatch):
    monkeypatch.setattr(store, "BOUND", 8)
    ws = [torch.full((2,), float(i)) for i in range(20)]
    for w in ws:
        store.derived("t", (w,), lambda w=w: w + 1)
    assert store.live() == 8
    assert all(store.ready("t", (w,)) for w in ws[-8:]) and not store.ready("t", (ws[0],))
    store.derived("t", (ws[12],), lambda: None)           # a hit moves the entry to the young end
    store.derived("t", (torch.zeros(3),), lambda: None)
    assert store.ready("t", (ws[12],)) and not store.ready("t", (ws[13],))
    assert store.RETIRED == []                              # nothing was pinned: evicted values are dropped
