"""The one cache of device operands derived from parameters (packed weights of the training convolutions)."""
import weakref

_id = id                   # the id lookup of the class (a test presents another tensor under a cached id through it)


class OperandCache(object):
    """value = f(owners) for a tuple of parameter tensors `owners` and a hashable `form` tag, valid for the owners' current
    VERSIONS.  One entry per (owners, form): a put for a new parameter version replaces the entry of the old one.

    What the users rely on:
      1. A hit needs the same owner OBJECTS (checked through weak references: an entry whose owner died, or whose id now belongs
         to another tensor, is never returned), the same `_version` and the same `data_ptr()` of every owner.  The optimiser's
         in-place update moves the version, `w.data = other` moves the storage; neither needs a clear().
      2. A hit returns the very object that was put, not a copy: conv_x3_dgrad writes the gradient scale into the header of the
         cached, shared operand, and captured graphs hold the addresses.
      3. A mark (ops.train_caches_mark) holds the cached tensors THEMSELVES for as long as it lives.  A mark of id()s alone failed:
         a put during the capture frees the replaced operand, CPython readily hands a freed object's id to a new one, and an
         operand made inside the capture then passed for a pre-existing one.
      4. keep_only(mark), right after a capture attempt, drops every entry whose allocation is not in the mark.  Entries made
         DURING a capture live in graph-pool memory and their packing kernels were only recorded: an eager step that found them
         would multiply by garbage (the captured step re-runs its packing kernels at every replay and needs no cache).  Entries
         from BEFORE it that were hits during it have their eager-pool addresses baked into the graph: they stay, and the owner of
         the graph pins every marked tensor for the graph's lifetime — clearing them at capture time was a use-after-free: the
         next eager allocation took the memory the replays read.  So clear() and an overflow cannot invalidate a graph either.
      5. At most `max_entries` entries, so that dead owners cannot accumulate: a put into a full cache empties it first.  4096,
         the larger of the bounds of the dictionaries this class replaced: a network holds a few hundred operands.
    forms_seen(owner) — every form ever put for `owner` alone — is bookkeeping, not a cache: it survives clear()."""

    def __init__(self, max_entries=4096):
        self.max_entries = max_entries
        self._entries = {}          # (form, id(owner), ...) -> ([(weakref, version, data_ptr) per owner], value, allocation)
        self._seen = {}             # id(owner) -> (weakref, {form, ...})

    def get(self, owners, form):
        """The value put for (owners, form) if every owner is still that object at that version and address (1), else None."""
        if len(owners) == 1:        # a layer's own operand, hundreds of hits in an eager step: no key unpacking, no loop
            w = owners[0]
            e = self._entries.get((form, _id(w)))
            if e is None:
                return None
            ref, version, ptr = e[0][0]
            return e[1] if ref() is w and w._version == version and w.data_ptr() == ptr else None
        e = self._entries.get((form, *map(_id, owners)))
        if e is None:
            return None
        for w, (ref, version, ptr) in zip(owners, e[0]):
            if ref() is not w or w._version != version or w.data_ptr() != ptr:
                return None
        return e[1]

    def put(self, owners, form, value, alloc=None):
        """Store and return `value`; `alloc`: the one device allocation behind it where that is another tensor (a list of views)."""
        if len(self._entries) >= self.max_entries:
            self._entries.clear()
        self._entries[(form, *map(_id, owners))] = ([(weakref.ref(w), w._version, w.data_ptr()) for w in owners], value,
                                                    value if alloc is None else alloc)
        if len(owners) == 1:
            seen = self._seen.get(_id(owners[0]))
            if seen is None or seen[0]() is not owners[0]:
                if len(self._seen) >= self.max_entries:
                    self._seen.clear()
                seen = self._seen[_id(owners[0])] = (weakref.ref(owners[0]), set())
            seen[1].add(form)
        return value

    def forms_seen(self, owner):
        seen = self._seen.get(_id(owner))
        return frozenset(seen[1]) if seen is not None and seen[0]() is owner else frozenset()

    def tensors(self):
        """The allocation of every entry."""
        return [e[2] for e in self._entries.values()]

    def keep_only(self, mark):
        """Drop the entries whose allocation is not in `mark` ({id(tensor): tensor})."""
        for k in [k for k, e in self._entries.items() if mark.get(id(e[2])) is not e[2]]:
            del self._entries[k]

    def clear(self):
        self._entries.clear()

    def __len__(self):
        return len(self._entries)
