"""Controlled memory for the tests: every buffer the package allocates uninitialised, with a chosen content and guards around it.

The package works in memory that is never clean in production: `_lib.workspace` hands out a cached, growing `torch.empty` buffer per
(device, stream, tag), and every output, gradient and temporary is a `torch.empty` of the caching allocator.  `controlled_memory`
replaces `torch.empty`, `torch.empty_like` and `_lib.workspace` (through `monkeypatch.setattr`: the package reaches them as attribute
look-ups at the call, tests/test_mem_table.py scans the sources for any other way) so that each such buffer is a view into a larger
byte buffer

    [ guard | payload | guard ]

whose payload starts at a multiple of 256 bytes (what the caching allocator and the library's own carving give: docs/WORKSPACE.md) and
whose every byte -- guards and payload -- holds the fill byte.  Pinned host allocations are filled and not guarded.  A kernel that
reads a region before anybody wrote it then reads the fill; one that writes past the end of a buffer writes into a guard.

Fill bytes (FILLS):
  0x00  clean: the baseline
  0xFF  NaN in float16 / float32 / float64, -1 as an int, all-ones tags
  0x7F  3.4e38 in float32, 1.4e306 in float64: finite, so visible to max-reductions and selects that drop a NaN; a large positive int
        -- a counter that looks as if everybody had arrived
  0x3C  small plausible floats (0.0115 in float32, 1.6e-18 in float64, 1.06 in float16): a contribution that leaks changes low bits
        instead of blowing up

The replaced `_lib.workspace` keeps the original's key, its grow-only rule and its `_ws_uses` accounting (the backward made ahead of
the cotangent recognises its buffer by that count).  fill=None leaves the content of the cached workspaces alone -- the run then works
in what the previous call left there ("stale") -- while torch allocations are filled with `torch_fill`; a cached workspace that has
to grow then keeps its old content at the head of the new buffer (the control words lie at the front of every layout), the rest
holds `torch_fill`.

No conftest, no pytest setting, no preloaded library; works on CPU tensors (tests/test_mem_table.py tests it there).
"""
import contextlib
import os
import sys

import torch

FILLS = {"00": 0x00, "FF": 0xFF, "7F": 0x7F, "3C": 0x3C}
ALIGN = 256
_HERE = os.path.abspath(__file__)
_real_empty, _real_empty_like = torch.empty, torch.empty_like

# one record per guarded allocation: dict(base, off, nbytes, guard, fill, site, kind)
_records = []
_ws_records = {}        # workspace key -> record (they outlive a context: the stale mode works on the previous context's buffers)
_inputs = []            # (guarded tensor, snapshot, site)
_state = dict(active=False, unguarded=[], ws_reused=0, ws_created=0, ws_grown=0, tags_created=set(), tags_stale=set())


def _site():
    """file:line of the nearest frame outside this module (and outside pytest's monkeypatch / contextlib)"""
    f = sys._getframe(1)
    while f is not None:
        fn = f.f_code.co_filename
        if os.path.abspath(fn) != _HERE and "contextlib" not in fn:
            return f"{os.path.relpath(fn, os.path.dirname(os.path.dirname(_HERE)))}:{f.f_lineno}"
        f = f.f_back
    return "?"


def _raw(nbytes, device, fill, guard, kind, site, pin=False):
    """A guarded byte buffer -> record; rec['payload'] is the uint8 view of the payload."""
    total = guard + nbytes + guard + ALIGN
    base = _real_empty(total, dtype=torch.uint8, device=device)
    base.fill_(fill)
    off = guard + (-(base.data_ptr() + guard)) % ALIGN
    rec = dict(base=base, off=off, nbytes=nbytes, guard=guard, fill=fill, site=site, kind=kind)
    rec["payload"] = base[off:off + nbytes]
    return rec


def _shape_of(size):
    if len(size) == 1 and not isinstance(size[0], int):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _guarded_tensor(shape, dtype, device, fill, guard, kind, requires_grad=False):
    esize = _real_empty((), dtype=dtype).element_size()
    rec = _raw(_numel(shape) * esize, device, fill, guard, kind, _site())
    _records.append(rec)
    t = rec["payload"].view(dtype).view(shape)
    return t.requires_grad_() if requires_grad else t


def _plain_filled(t, fill):
    """an allocation the harness cannot guard (pinned, exotic layout): filled all the same"""
    if t.numel():
        flat = t.view(-1) if t.is_contiguous() else None
        if flat is not None:
            flat.view(torch.uint8).fill_(fill)
    return t


def _make_empty(fill, guard):
    def empty(*size, dtype=None, device=None, pin_memory=False, requires_grad=False, **kw):
        dtype = torch.get_default_dtype() if dtype is None else dtype
        if not size and "size" in kw:
            size = (kw.pop("size"),)
        if pin_memory or kw.get("out") is not None or kw.get("layout", torch.strided) is not torch.strided or \
                kw.get("memory_format", torch.contiguous_format) is not torch.contiguous_format or kw.get("names") is not None:
            t = _real_empty(*size, dtype=dtype, device=device, pin_memory=pin_memory, requires_grad=requires_grad, **kw)
            if not pin_memory:
                _state["unguarded"].append(_site())
            return _plain_filled(t, fill)
        device = torch.device("cpu" if device is None else device)
        return _guarded_tensor(_shape_of(size), dtype, device, fill, guard, "empty", requires_grad)

    def empty_like(t, dtype=None, device=None, requires_grad=False, **kw):
        if kw.get("memory_format", torch.preserve_format) not in (torch.preserve_format, torch.contiguous_format) or \
                kw.get("layout", torch.strided) is not torch.strided or (not t.is_contiguous() and "memory_format" not in kw):
            _state["unguarded"].append(_site())
            return _plain_filled(_real_empty_like(t, dtype=dtype, device=device, requires_grad=requires_grad, **kw), fill)
        return _guarded_tensor(tuple(t.shape), t.dtype if dtype is None else dtype, t.device if device is None else torch.device(device),
                               fill, guard, "empty_like", requires_grad)
    return empty, empty_like


def _make_workspace(_lib, fill, torch_fill, guard):
    def workspace(device, nbytes, tag, stream=None):
        key = (device.index, _lib.current_stream_handle(device) if stream is None else stream, tag)
        with _lib._ws_lock:
            buf = _lib._ws_cache.get(key)
            if buf is None or buf.numel() < nbytes:
                rec = _raw(int(nbytes), device, torch_fill if fill is None else fill, guard, "workspace:" + str(tag), _site())
                if buf is not None and fill is None:
                    # stale mode, the buffer has to grow: what the old one held stays at the head of the new one (the status block,
                    # the counter ring and the per-problem words lie at the front of every layout), the rest holds torch_fill
                    rec["payload"][:buf.numel()].copy_(buf)
                    _state["ws_grown"] += 1
                    _state["tags_stale"].add(tag)
                else:
                    _state["ws_created"] += 1
                    _state["tags_created"].add(tag)
                _ws_records[key] = rec
                buf = rec["payload"]
                _lib._ws_cache[key] = buf
            else:
                _state["ws_reused"] += 1
                if tag not in _state["tags_created"]:
                    _state["tags_stale"].add(tag)
            _lib._ws_uses[key] = _lib._ws_uses.get(key, 0) + 1
            return buf
    return workspace


def release(_lib):
    """Drop the cached workspaces and every record (the guards of dropped buffers are not checked any more)."""
    _lib.release_workspaces()
    _ws_records.clear()
    del _records[:]
    del _inputs[:]


@contextlib.contextmanager
def controlled_memory(monkeypatch, fill, guard_bytes=4096, torch_fill=0xFF):
    """Inside: torch.empty / torch.empty_like / _lib.workspace give guarded buffers filled with `fill` (an int 0..255).
    fill=None: the cached workspaces keep what they hold (and their guards), torch allocations are filled with `torch_fill`;
    otherwise the cached workspaces are released on entry.  Yields the counters: ws_created / ws_reused / ws_grown (hand-outs of a
    new buffer, of a cached one, of a larger one that took over a cached one's content: fill=None only), tags_created (tags whose
    buffer was made inside), tags_stale (tags handed out with content from before the context), unguarded (call sites)."""
    from lqp_py_amd import _lib
    assert fill is None or 0 <= int(fill) <= 255
    assert not _state["active"], "controlled_memory does not nest"
    if fill is not None:
        _lib.release_workspaces()
        _ws_records.clear()
    _state.update(ws_reused=0, ws_created=0, ws_grown=0, unguarded=[], tags_created=set(), tags_stale=set())
    empty, empty_like = _make_empty(torch_fill if fill is None else int(fill), guard_bytes)
    with monkeypatch.context() as mp:
        mp.setattr(torch, "empty", empty)
        mp.setattr(torch, "empty_like", empty_like)
        mp.setattr(_lib, "workspace", _make_workspace(_lib, fill, torch_fill, guard_bytes))
        _state["active"] = True
        try:
            yield _state
        finally:
            _state["active"] = False


def guarded(t, fill=0xFF, guard_bytes=4096, offset_elems=0):
    """A copy of the input tensor `t` inside its own guarded buffer (same shape, dtype, device, and strides where `t` is a dense
    permutation), remembered for check_inputs_untouched.  offset_elems=k: the copy starts k elements behind the 256-byte aligned
    payload start -- `flat[k:k + numel].view(shape)`, an address that is element-aligned only."""
    if t is None:
        return None
    t = t.detach()
    numel, esize = t.numel(), t.element_size()
    rec = _raw((numel + offset_elems) * esize, t.device, fill, guard_bytes, "input", _site())
    _records.append(rec)
    flat = rec["payload"].view(t.dtype)[offset_elems:offset_elems + numel]
    dense = t.is_contiguous() or (numel and sum((s - 1) * st for s, st in zip(t.shape, t.stride())) == numel - 1)
    g = flat.view(t.shape) if t.is_contiguous() else (flat.as_strided(t.shape, t.stride()) if dense else flat.view(t.shape))
    g.copy_(t)
    _inputs.append((g, g.clone(), rec["site"]))
    return g


def _bad_bytes(view, fill):
    return (view != fill).nonzero().flatten()


def check_guards():
    """-> every allocation with a guard byte that changed: dict(site, kind, side ("front" | "back"), first (offset of the first changed
    byte: back guards count from the end of the payload, front guards back from its start), count)."""
    out = []
    for rec in list(_records) + list(_ws_records.values()):
        base, off, nb, fill = rec["base"], rec["off"], rec["nbytes"], rec["fill"]
        for side, view in (("front", base[:off]), ("back", base[off + nb:])):
            if bool((view != fill).any()):
                bad = _bad_bytes(view, fill)
                first = int(bad[0]) if side == "back" else off - 1 - int(bad[-1])
                out.append(dict(site=rec["site"], kind=rec["kind"], side=side, first=first, count=int(bad.numel()), nbytes=nb))
    return out


def check_inputs_untouched():
    """-> the call sites of the `guarded` inputs whose bytes differ from what they held when they were made"""
    out = []
    for g, snap, site in _inputs:
        a, b = g.detach().contiguous().view(-1).view(torch.uint8), snap.contiguous().view(-1).view(torch.uint8)
        if not torch.equal(a, b):
            out.append(dict(site=site, changed=int((a != b).sum())))
    return out


def forget():
    """Forget the records of torch allocations and inputs made so far (workspaces stay): between the runs of one test item."""
    del _records[:]
    del _inputs[:]


def same_bits(a, b):
    """bitwise equality of two tensors (NaN == NaN with the same payload), of None with None, or of two non-tensors"""
    if a is None or b is None:
        return a is None and b is None
    if not torch.is_tensor(a):
        return (not torch.is_tensor(b)) and a == b
    if not torch.is_tensor(b) or a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))
