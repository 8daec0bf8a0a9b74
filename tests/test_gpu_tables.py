"""GPU: dvc_amd.tables.Staging, pack and upload as a unit — four uploads in a row through one Staging with nothing synchronised
between them: the slot flips every time, the first two allocate their buffers with a quarter to spare, the third and fourth
rewrite those buffers behind `acquire`, and every table holds exactly what was packed for it.  It runs the flip, the grow and the
event wait together; it does not prove the wait, since a copy this small has normally run long before its buffer is rewritten."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_four_unsynchronised_uploads_through_one_staging_keep_their_bytes():
    from dvc_amd import tables
    device = torch.device("cuda", torch.cuda.current_device())
    st = tables.Staging()
    sent, slots = [], []
    for i, nbytes in enumerate((96, 4096, 64, 4096)):
        head = np.random.default_rng(i).integers(0, 256, nbytes // 2, dtype=np.uint8)       # two arrays, distinct per upload
        tail = np.full(nbytes - nbytes // 2, 0x11 * (i + 1), dtype=np.uint8)
        slot = st.acquire(nbytes)
        assert st.buf[slot].is_pinned() and st.buf[slot].numel() >= nbytes
        offsets, total = tables.pack(st.buf[slot].numpy(), [head, tail])
        assert list(offsets) == [0, nbytes // 2] and total == nbytes
        table = tables.upload(st.buf[slot], nbytes, device, extra=8 * (i % 2))
        st.sent(slot)
        assert table.numel() == nbytes + 8 * (i % 2) and table.device == device
        sent.append((table, nbytes, head.tobytes() + tail.tobytes()))
        slots.append(slot)
    assert slots == [1, 0, 1, 0] and st.slot == 0
    assert st.buf[1].numel() == 96 + 96 // 4 and st.buf[0].numel() == 4096 + 4096 // 4      # grown once each, by a quarter
    for table, nbytes, expect in sent:
        assert table[:nbytes].cpu().numpy().tobytes() == expect
