"""A batch of 65,536 + 7 files: the host tables are counted and filled over 64 file ranges on host
threads (bw_plan.h) instead of one walk.  tests/test_plan.py compares those tables with a serial
walk on the CPU; here the batch they describe goes through the GPU, record for record against the
oracle.

Nearly all files hold 0-48 bytes; five files of a few KiB, the first and the last file among them,
are CDC files (min 64, avg 256, max 1024, small-file threshold 256), so CDC units lie between small
ones across the borders of the ranges.  Under 4 MiB of data in all.

BW_OPT_SPLIT is not run on this list: a batch is split only from 64 MiB of file data on, and no
option lowers that threshold.
"""
import numpy as np
import pytest

from backuwup_amd import Context, make_params
from backuwup_amd.synth import splitmix_bytes

pytestmark = pytest.mark.gpu

PARAMS, THRESHOLD = (64, 256, 1024), 256
NF = 65536 + 7
BIG = {0: 5000, 1024: 3333, 30000: 9001, 65535: 2049, NF - 1: 4097}  # file -> bytes; 1024: a range's first file


def test_many_files_match_oracle(oracle):
    import torch
    rng = np.random.default_rng(77)
    lens = rng.integers(0, 49, NF).astype(np.uint64)
    for f, n in BIG.items():
        lens[f] = n
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    total = int(lens.sum())
    assert total < 4 << 20 and int((lens == 0).sum()) > 1000
    # few distinct byte patterns among the tiny files: most of them are duplicates of earlier ones
    data = splitmix_bytes(5, total)
    for f in np.nonzero(lens < 8)[0]:
        data[int(offs[f]):int(offs[f] + lens[f])] = f % 3
    want = oracle.process_files(data, offs, lens, *PARAMS, small_threshold=THRESHOLD, threads=8)
    assert len(want) > NF and 0 < int(want["is_dup"].sum()) < len(want)
    dev = torch.from_numpy(data).cuda()
    torch.cuda.synchronize()
    with Context(0) as c:
        c.index_reset()
        c.submit_device(dev.data_ptr(), total, offs, lens, make_params(*PARAMS, small_file_threshold=THRESHOLD))
        got = c.results()
        geo = c.batch_counters()
    assert got.shape == want.shape
    for field in ("file", "offset", "length", "gear_hash", "is_dup"):
        assert np.array_equal(got[field], want[field]), field
    assert np.array_equal(got["digest"], want["digest"])
    assert geo["cdc_files"] == len(BIG)
    assert geo["segments"] == sum(-(-n // 2048) for n in BIG.values())  # small batch: 2 x max per segment
