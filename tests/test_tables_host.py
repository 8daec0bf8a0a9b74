"""CPU: dvc_amd.tables without a device — `pack` lays the record arrays of every table family out where the code before it did,
keeps every chunk table 16-byte aligned, writes exactly the arrays' bytes and can leave an unchanged tail alone; `Resident.use`
keeps a captured table once and tells the allocator about a stream change only for a table no graph holds."""
import itertools

import numpy as np
import pytest
import torch

COUNTS = (0, 1, 3)


def _families():
    from dvc_amd import losses, optim
    return {"adam": (optim.TENSOR_DTYPE, optim.CHUNK_DTYPE),
            "capturable": (optim.TENSOR_DTYPE, optim.CHUNK_DTYPE, optim.ADVANCE_DTYPE),
            "fused": (losses.TERM_DTYPE, losses.CHUNK_DTYPE),
            "plan": (losses.PLAN_TERM_DTYPE, losses.CHUNK_DTYPE)}


def _records(dtype, n, seed):
    raw = np.random.default_rng(seed).integers(0, 256, n * dtype.itemsize, dtype=np.uint8)
    return raw.view(dtype)


@pytest.mark.parametrize("family", ["adam", "capturable", "fused", "plan"])
def test_pack_offsets_alignment_and_bytes(family):
    from dvc_amd import tables
    dtypes = _families()[family]
    for ns in itertools.product(COUNTS, repeat=len(dtypes)):
        arrays = [_records(dt, n, 7 * i + n) for i, (dt, n) in enumerate(zip(dtypes, ns))]
        t_bytes, c_bytes = ns[0] * dtypes[0].itemsize, ns[1] * dtypes[1].itemsize
        old = [0, t_bytes, t_bytes + c_bytes][:len(dtypes)]             # where the call sites put them before `pack`
        total = sum(n * dt.itemsize for dt, n in zip(dtypes, ns))
        host = np.full(total + 32, 0xA5, dtype=np.uint8)
        offsets, end = tables.pack(host, arrays)
        assert list(offsets) == old and end == total, (family, ns, offsets, end)
        assert offsets[1] % 16 == 0, (family, ns)                       # the chunk table
        if len(dtypes) == 3:
            assert offsets[2] % 16 == 0 and end % 8 == 0, (family, ns)  # the advance table; scratch behind it holds doubles
        assert host[:end].tobytes() == b"".join(a.tobytes() for a in arrays), (family, ns)
        assert (host[end:] == 0xA5).all(), (family, ns)                 # nothing behind the tables is touched
        for a, at in zip(arrays, offsets):                              # and each array reads back as itself
            assert host[at:at + a.nbytes].view(a.dtype).tobytes() == a.tobytes()


def test_record_sizes_that_keep_the_chunk_table_aligned():
    from dvc_amd import losses, optim
    assert optim.TENSOR_DTYPE.itemsize == losses.TERM_DTYPE.itemsize == 80 and losses.PLAN_TERM_DTYPE.itemsize == 112
    assert optim.CHUNK_DTYPE.itemsize == losses.CHUNK_DTYPE.itemsize == 16 and optim.ADVANCE_DTYPE.itemsize == 40


@pytest.mark.parametrize("family", ["adam", "fused"])
@pytest.mark.parametrize("n, n_c", [(1, 1), (3, 3), (3, 0), (1, 3)])
def test_pack_leaves_an_unchanged_tail_in_place(family, n, n_c):
    from dvc_amd import tables
    rec_dt, chunk_dt = _families()[family]
    first, second, chunks = _records(rec_dt, n, 1), _records(rec_dt, n, 2), _records(chunk_dt, n_c, 3)
    host = np.full(first.nbytes + chunks.nbytes + 16, 0x5A, dtype=np.uint8)
    offsets, end = tables.pack(host, [first, chunks])
    again, end_again = tables.pack(host, [second], tail_bytes=chunks.nbytes)
    assert end_again == end == first.nbytes + chunks.nbytes
    assert list(offsets) == [0, first.nbytes] and list(again) == [0]
    assert host[:end].tobytes() == second.tobytes() + chunks.tobytes()          # new records, the OLD chunk bytes
    assert (host[end:] == 0x5A).all()


# ---- Resident.use
class _Table:
    def __init__(self):
        self.recorded = []

    def record_stream(self, stream):
        self.recorded.append(stream)


@pytest.fixture
def current_stream(monkeypatch):
    """torch.cuda.current_stream() without a device: a marker object that `use` hands to record_stream."""
    marker = object()
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: marker)
    return marker


def test_resident_captured_once_is_appended_once(current_stream):
    from dvc_amd import tables
    res, kept = tables.Resident("key", _Table(), None, 11), []
    assert (res.key, res.pinned, res.stream, res.captured) == ("key", None, 11, False)
    res.use(kept, True, 11)
    res.use(kept, True, 11)
    res.use(kept, True, 12)                 # a capture on another stream: still one entry, and nothing for the allocator
    assert kept == [res] and res.captured and res.table.recorded == []


def test_resident_stream_change_uncaptured_is_one_record_stream(current_stream):
    from dvc_amd import tables
    res, kept = tables.Resident("key", _Table(), None, 11), []
    res.use(kept, False, 11)                # the stream it was built on: nothing
    assert res.table.recorded == [] and res.stream == 11
    res.use(kept, False, 12)
    res.use(kept, False, 12)                # the same stream again: not recorded twice
    assert res.table.recorded == [current_stream] and res.stream == 12 and kept == [] and not res.captured


def test_resident_stream_change_captured_is_no_record_stream(current_stream):
    from dvc_amd import tables
    res, kept = tables.Resident("key", _Table(), "pinned", 11), []
    res.use(kept, True, 11)
    res.use(kept, False, 12)                # eager use of a captured table on another stream: the graph keeps it alive
    assert res.table.recorded == [] and res.stream == 12 and kept == [res] and res.pinned == "pinned"


def test_owner_records_are_residents():
    from dvc_amd import losses, optim, tables
    assert issubclass(optim._Resident, tables.Resident) and issubclass(losses._PlanResident, tables.Resident)
    assert optim._Staging is tables.Staging
