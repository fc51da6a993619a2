"""Tensors derived from model weights (MFMA fragment layouts, BatchNorm / LayerNorm folds, concatenated heads, padded copies, the
pyramid's zero-input response), built once and reused until a source changes.  One store, one policy (end of section 2):

  * a slot is (tag, per-source (data_ptr, shape, dtype, device), extra); its entry holds the sources' `_version`s, the value and
    strong references to the sources, so a source's address cannot be reused by another tensor while the entry exists;
  * a lookup whose versions are stale rebuilds the value under no_grad and replaces the entry in its slot;
  * a value handed out while the current stream is capturing a HIP graph is PINNED: the graph has its address baked in, so when
    the entry is later replaced or evicted a pinned value is retired (kept alive for the life of the process), an unpinned one
    is dropped;
  * a value BUILT while capturing only has its build kernels recorded, not run: it is returned and retired, but not stored, so
    the next eager call builds it again;
  * one LRU bound over the whole store.

Depends on torch only."""
import collections

import torch

BOUND = 2048            # entries over the whole store: 6x what the 5-agent scene keeps live
RETIRED = []            # kept alive, never freed: a captured graph may still read them (shared with ops._workspace)
builds = 0              # values built so far (tests: a repeated eager step must build none)

_STORE = collections.OrderedDict()      # slot -> _Entry, least recently used first


class _Entry:
    __slots__ = ("versions", "value", "sources", "pinned")

    def __init__(self, versions, value, sources):
        self.versions, self.value, self.sources, self.pinned = versions, value, sources, False


def capturing():
    """True while the current stream is capturing a graph (its own function so that CPU tests can patch it)."""
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


def retire(*tensors):
    """Keep `tensors` (or values holding them) alive for good."""
    RETIRED.extend(tensors)


def _slot(tag, sources, extra):
    return (tag, extra, *[None if s is None else (s.data_ptr(), s.shape, s.dtype, s.device) for s in sources])


def _versions(sources):
    return [None if s is None else s._version for s in sources]


def _drop(entry):
    if entry.pinned:
        retire(entry.value)


def ready(tag, sources, extra=()):
    """True if a valid entry exists for the current contents of `sources` (the capture guards ask this before a build)."""
    e = _STORE.get(_slot(tag, sources, extra))
    return e is not None and e.versions == _versions(sources)


def derived(tag, sources, build, extra=()):
    """build() for the current contents of `sources` (tensors; None allowed), cached."""
    global builds
    slot = _slot(tag, sources, extra)
    versions = _versions(sources)
    e = _STORE.get(slot)
    if e is not None and e.versions == versions:
        _STORE.move_to_end(slot)
        if not e.pinned and capturing():
            e.pinned = True
        return e.value
    with torch.no_grad():
        value = build()
    builds += 1
    if capturing():
        retire(value)
        return value
    if e is not None:
        _drop(e)
    _STORE[slot] = _Entry(versions, value, tuple(sources))
    _STORE.move_to_end(slot)
    while len(_STORE) > BOUND:
        _drop(_STORE.popitem(last=False)[1])
    return value


def live():
    """Number of entries in the store."""
    return len(_STORE)
