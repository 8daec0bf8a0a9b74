"""How the small host tables of dvc_amd.optim and dvc_amd.losses reach the device ("Host tables", has the reasons):
records are `pack`ed into PINNED memory and `upload`ed with one non-blocking copy on the current stream, which reads the bytes when
the stream gets to it.  So an eager upload goes through a `Staging`, which never rewrites a buffer before its copy ran; a CAPTURED
upload, whose copy node reads again on every replay, goes from a pinned buffer of its own that is never rewritten (the owner's
spare, kept in `Resident.pinned`).  Tables that stay on the device between calls are a `Resident`.  numpy and torch only."""
import torch


class Staging:
    """Two pinned buffers used in turn; `event[i]` is recorded after the copy out of buffer i."""

    def __init__(self):
        self.buf = [None, None]
        self.event = [None, None]
        self.counts = [None, None]      # the counts whose chunk table buffer i holds (at the offset they imply); the owner's to set
        self.slot = 0

    def acquire(self, nbytes):
        """Flip to the other buffer, wait until the copy that last read it has run, make it hold `nbytes` -> its slot."""
        slot = self.slot = 1 - self.slot
        if self.event[slot] is not None:
            self.event[slot].synchronize()
        if self.buf[slot] is None or self.buf[slot].numel() < nbytes:
            self.buf[slot] = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, pin_memory=True)
            self.counts[slot] = None
        return slot

    def sent(self, slot):
        """Call after enqueueing the copy out of buffer `slot`, on the stream it was enqueued on."""
        if self.event[slot] is None:
            self.event[slot] = torch.cuda.Event()
        self.event[slot].record()


def pack(host, arrays, tail_bytes=0):
    """Write the structured `arrays` back to back into `host`, the uint8 numpy view of a pinned buffer: the layout
    [records | chunk records | more] of every table here.  -> (the byte offset of each array, the total).  `tail_bytes` stands for
    one more array of that size which `host` already holds behind them (a chunk table whose counts did not change): its bytes are
    left alone and counted in the total.

    Nothing is padded; the records' sizes keep what follows them aligned: DvcAdamTensor and DvcLossTerm are 80 bytes, DvcPlanTerm
    112 and a chunk record 16, so a chunk table behind any number of records starts at a multiple of 16, and so does what follows
    it (advance records, a plan's float64 scratch); behind the 40-byte DvcAdamAdvance records the scratch is still 8-byte aligned."""
    offsets, at = [], 0
    for a in arrays:
        host[at:at + a.nbytes].view(a.dtype)[:] = a
        offsets.append(at)
        at += a.nbytes
    return offsets, at + tail_bytes


def upload(pinned, nbytes, device, extra=0):
    """One allocation and one non-blocking copy on the current stream: `pinned[:nbytes]`, then `extra` bytes of uninitialised scratch."""
    table = torch.empty(nbytes + extra, dtype=torch.uint8, device=device)
    (table[:nbytes] if extra else table).copy_(pinned[:nbytes], non_blocking=True)      # (no scratch: no slice, the call as it was)
    return table


class Resident:
    """A table tensor that stays on the device and what it was built from (`key`: its owner's fingerprint)."""
    __slots__ = ("key", "table", "pinned", "stream", "captured")

    def __init__(self, key, table, pinned, stream):
        self.key, self.table = key, table
        self.pinned = pinned        # the buffer a CAPTURED upload reads on every replay (None for an eager upload)
        self.stream = stream        # the handle of the last stream it was used on
        self.captured = False

    def use(self, captured_list, capturing, stream):
        """Before launching on the table on the current stream, whose handle is `stream`.  Under capture a graph refers to the table
        from now on: it joins `captured_list` (read only then), once, and lives as long as that list's owner.  Otherwise, on another
        stream than the last, the allocator is told not to reuse the table under this stream's launches — unless a graph holds it."""
        if capturing:
            if not self.captured:
                self.captured = True
                captured_list.append(self)
        elif stream != self.stream:
            if not self.captured:
                self.table.record_stream(torch.cuda.current_stream())
            self.stream = stream
