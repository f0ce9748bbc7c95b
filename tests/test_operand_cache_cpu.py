"""upflow_pytorch_amd._operand_cache.OperandCache — the one version-keyed cache of the training path's packed operands — on CPU
tensors: what is a hit, what is never one, what survives a clear and an overflow."""
import torch

from upflow_pytorch_amd import _operand_cache
from upflow_pytorch_amd._operand_cache import OperandCache

FORM = ('pack', torch.bfloat16, 0)


def _w():
    return torch.zeros(4, 4, 3, 3)


def test_hit_returns_the_object_and_a_new_version_misses():
    c, w, v = OperandCache(), _w(), torch.zeros(8)
    assert c.get((w,), FORM) is None
    assert c.put((w,), FORM, v) is v
    assert c.get((w,), FORM) is v and c.get((w,), FORM) is v                 # the object itself, every time
    assert c.get((w,), ('pack', torch.bfloat16, 1)) is None and c.get((w, w), FORM) is None
    before = w._version
    with torch.no_grad():
        w.add_(0)
    assert w._version == before + 1                                          # the in-place update moved the version
    assert c.get((w,), FORM) is None
    v2 = torch.ones(8)
    c.put((w,), FORM, v2)
    assert c.get((w,), FORM) is v2 and len(c) == 1 and c.tensors() == [v2]   # the new version replaced the old entry


def test_data_surgery_misses_and_a_new_put_leaves_one_entry():
    c, w, v = OperandCache(), _w(), torch.zeros(8)
    c.put((w,), FORM, v)
    before, ptr = w._version, w.data_ptr()
    w.data = torch.ones(4, 4, 3, 3)
    assert w._version == before and w.data_ptr() != ptr                      # the storage moved, the version did not
    assert c.get((w,), FORM) is None
    v2 = torch.ones(8)
    c.put((w,), FORM, v2)
    assert c.get((w,), FORM) is v2 and len(c) == 1 and c.tensors() == [v2]


def test_six_owner_entries_miss_when_any_owner_moves():
    form = ('stacks', ((0, 4, 1), (4, 4, 2)), torch.float16)
    for moved in range(6):
        for surgery in (False, True):
            c, ws = OperandCache(), tuple(_w() for _ in range(6))
            pool = torch.zeros(16)
            views = [pool[:8], pool[8:]]
            assert c.put(ws, form, views, alloc=pool) is views
            assert c.get(ws, form) is views and c.tensors() == [pool] and c.tensors()[0] is pool
            assert c.get(ws[:5], form) is None and c.get(ws[::-1], form) is None
            if surgery:
                ws[moved].data = torch.ones(4, 4, 3, 3)
            else:
                with torch.no_grad():
                    ws[moved].add_(0)
            assert c.get(ws, form) is None, (moved, surgery)
            assert all(c.forms_seen(w) == frozenset() for w in ws)           # (only single-owner forms are remembered)


def test_an_entry_is_not_returned_for_another_tensor_under_the_same_id(monkeypatch):
    c, w, other, w6 = OperandCache(), _w(), _w(), tuple(_w() for _ in range(6))
    v, v6 = torch.zeros(8), torch.zeros(8)
    c.put((w,), FORM, v)
    c.put(w6, FORM, v6)
    # `other` (same shape, same version, and — below — the same address) is presented under w's id, as after CPython recycled it
    alias = {id(other): id(w)}
    monkeypatch.setattr(_operand_cache, '_id', lambda t: alias.get(id(t), id(t)))
    assert other._version == w._version
    assert c.get((w,), FORM) is v and c.get((other,), FORM) is None and c.forms_seen(other) == frozenset()
    assert c.get(w6, FORM) is v6
    for i in range(6):
        alias = {id(other): id(w6[i])}
        assert c.get(w6[:i] + (other,) + w6[i + 1:], FORM) is None
    # the owner dies, its id is taken over: the dead entry is not returned, a put for the new tensor replaces it
    alias = {id(other): id(w)}
    del w
    assert c.get((other,), FORM) is None and c.forms_seen(other) == frozenset()
    v2 = torch.ones(8)
    c.put((other,), FORM, v2)
    assert c.get((other,), FORM) is v2 and len(c) == 2 and c.forms_seen(other) == {FORM}


def test_same_address_is_not_enough():
    """A view of the owner's storage has its data_ptr and (shared counter) its version, and is still another object."""
    c, w, v = OperandCache(), _w(), torch.zeros(8)
    c.put((w,), FORM, v)
    view = w.view(4, 4, 3, 3)
    assert view.data_ptr() == w.data_ptr() and view._version == w._version
    assert c.get((view,), FORM) is None and c.get((w,), FORM) is v


def test_keep_only_and_tensors():
    c, a, b = OperandCache(), _w(), _w()
    va, vb = torch.zeros(8), torch.zeros(8)
    c.put((a,), FORM, va)
    mark = {id(t): t for t in c.tensors()}
    c.put((b,), FORM, vb)
    assert sorted(map(id, c.tensors())) == sorted(map(id, (va, vb)))
    c.keep_only(mark)
    assert c.tensors() == [va] and c.tensors()[0] is va and c.get((a,), FORM) is va and c.get((b,), FORM) is None
    # an equal id is not enough: the mark must hold that very tensor
    c.keep_only({id(va): vb})
    assert len(c) == 0


def test_forms_seen_survives_clear():
    c, w = OperandCache(), _w()
    c.put((w,), FORM, torch.zeros(8))
    c.put((w,), ('x3', True), torch.zeros(8))
    c.clear()
    assert len(c) == 0 and c.get((w,), FORM) is None
    assert c.forms_seen(w) == {FORM, ('x3', True)} and c.forms_seen(_w()) == frozenset()


def test_overflow_bound_leaves_the_cache_usable():
    assert OperandCache().max_entries == 4096
    c = OperandCache(max_entries=8)
    owners = [_w() for _ in range(30)]
    for i, w in enumerate(owners):
        v = torch.full((2,), float(i))
        assert c.put((w,), FORM, v) is v
        assert c.get((w,), FORM) is v and 1 <= len(c) <= 8 and len(c._seen) <= 8
    assert c.forms_seen(owners[-1]) == {FORM}
    dead = [c.put((_w(),), FORM, torch.zeros(2)) for _ in range(100)]        # owners that die at once cannot pile up
    assert len(dead) == 100 and len(c) <= 8 and len(c._seen) <= 8
