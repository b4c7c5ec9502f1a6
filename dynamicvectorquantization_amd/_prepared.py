"""Device buffers PREPARED from parameter tensors (codebook tile images, the conv folded into a codebook, gate-weight and
conv-weight images) and the module hooks that drop them: the one place that knows how such a buffer is shared by streams.
"""
import torch

from . import _lib


class PreparedImage:
    """One device buffer prepared from parameter tensors by a kernel, rebuilt when its key changes, safe when several streams
    use it (encode.StreamSlots drives one model from three).  The user makes the key -- (data_ptr, _version, shape, device) of
    the OWNING parameters: a write through `.data` does not bump the version, hence `invalidate()` -- and asks
    `lookup(key, device)`; on None it gives `rebuild` the byte count and a callable that launches the prepare kernel(s).

    The rules, all of them here:
      * a rebuild goes to a FRESH buffer; the replaced one is kept alive in `_retired` for the kernels other streams still
        have queued against it.  The last 4 are kept: the sites this class replaced kept 4 (codebook) or 2 (gate, conv) with
        no stated reason for the difference, so the more conservative figure holds everywhere;
      * the building stream records an event; any other stream waits for it before its first use; once the event has
        completed it is forgotten, and the steady state is one key comparison that makes no Stream object
        (torch.cuda.current_stream() alone is ~5 us of every call: tools/module_overhead.py).  Sites on a hot path test
        that state themselves -- `key == img.key and img._built is None`: `img.buf` is good as it is -- before they pay for
        a call of `lookup`; nothing else about the rules is theirs to know;
      * no event is queried while the stream is capturing (a capture is always preceded by uncaptured warm-up calls on the
        capturing stream: ordered there)."""

    def __init__(self):
        self.key = None
        self.buf = None
        self._built = None       # (stream handle, event) of the last build, until the event has completed
        self._retired = []       # replaced buffers other streams may still be reading

    def invalidate(self):
        self.key = None

    def retire(self, buf):
        """keep a replaced buffer (this image's, or one derived from it) alive for readers already queued"""
        if buf is not None:
            self._retired = (self._retired + [buf])[-4:]

    def adopt(self, other):
        """take over what `other` -- an image derived from this one that is being dropped -- keeps alive"""
        for buf in other._retired + [other.buf]:
            self.retire(buf)

    def lookup(self, key, device):
        """the buffer, ordered for the current stream of `device` -- or None: `key` is not what it was built for"""
        if key != self.key:
            return None
        b = self._built
        if b is not None and not torch.cuda.is_current_stream_capturing():
            if b[1].query():
                self._built = None                       # long done: nothing to order any more
            elif b[0] != _lib.stream_ptr(device):
                torch.cuda.current_stream(device).wait_event(b[1])
        return self.buf

    def rebuild(self, key, device, nbytes, launch, in_place=False):
        """launch(buffer pointer, buffer bytes, stream handle) queues the prepare kernel(s) on the current stream of `device`.
        in_place: overwrite the old buffer when it is large enough -- only for a caller that has ordered this stream behind
        every reader of it (_CodebookPrep in training mode)."""
        if not (in_place and self.buf is not None and self.buf.numel() >= nbytes and self.buf.device == device):
            self.retire(self.buf)
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        cur = torch.cuda.current_stream(device)
        with _lib.on_device(device):
            launch(self.buf.data_ptr(), self.buf.numel(), cur.cuda_stream)
            ev = torch.cuda.Event()
            ev.record(cur)
        self._built = (cur.cuda_stream, ev)
        self.key = key
        return self.buf


class InvalidatesPrepared:
    """nn.Module mixin (listed BEFORE the nn.Module base): `load_state_dict` and `.to()` / `.cuda()` / `.float()` invalidate
    the prepared images named in `_prepared` (attributes with an `invalidate()`), after the parameters have their new values
    -- after `_apply` they are the new tensors."""
    _prepared = ()

    def _invalidate_prepared(self):
        for name in self._prepared:
            getattr(self, name).invalidate()

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._invalidate_prepared()

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._invalidate_prepared()
        return out
