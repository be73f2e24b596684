"""bench.py's command line: a plain run is lean (--full is off by default) and --dump-outputs
writes the last timed step's results as float arrays that hold every value exactly."""
import sys

import numpy as np
import torch

from conftest import REPO


def _bench():
    sys.path.insert(0, REPO)
    import bench
    return bench


def test_plain_run_is_the_default(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup) == (1, 3, 1)
    assert a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_holds_the_bitstream_and_the_batch_exactly(tmp_path):
    bench = _bench()
    from idfcodec.codec import Bitstream
    g = torch.Generator().manual_seed(0)
    nw = torch.randint(0, 50, (6,), generator=g).to(torch.int64)
    st = torch.randint(-(2 ** 63), 2 ** 63 - 1, (6,), generator=g, dtype=torch.int64)
    st[0], st[1] = -1, -(2 ** 63)  # u64 all ones, and the top bit alone
    w = torch.randint(-(2 ** 31), 2 ** 31 - 1, (int(nw.sum()),), generator=g, dtype=torch.int32)
    w[0] = -1
    bs = Bitstream(2, [(6, 32, 32), (12, 16, 16), (48, 8, 8)], st, nw, w)
    out = torch.randint(0, 256, (2, 3, 64, 64), generator=g, dtype=torch.uint8)
    d = tmp_path / "dump"
    bench.dump_outputs(str(d), bs, out)
    got = {p.name[:-4]: np.load(p, allow_pickle=False) for p in d.iterdir()}
    assert sorted(got) == ["bitstream_nwords", "bitstream_states_hi", "bitstream_states_lo",
                           "bitstream_words", "decoded"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    states = (got["bitstream_states_hi"].astype(np.uint64) << np.uint64(32)) \
        | got["bitstream_states_lo"].astype(np.uint64)
    assert np.array_equal(states.view(np.int64), st.numpy())
    assert np.array_equal(got["bitstream_nwords"].astype(np.int64), nw.numpy())
    assert np.array_equal(got["bitstream_words"].astype(np.uint32).view(np.int32), w.numpy())
    assert np.array_equal(got["decoded"].astype(np.uint8), out.numpy())
    assert got["decoded"].shape == (2, 3, 64, 64)
