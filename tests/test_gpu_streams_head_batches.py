"""egoego_s1_head_batch runs on the caller's stream, and only there (include/egoego_hip.h, Conventions): the batch
build under a side stream whose inputs (the packed tables, the sequence ids, the draw ids) arrive late, by the method of
tests/stream_cases.py.

A file of its own, collected behind tests/test_gpu_streams.py, for the reason tests/test_gpu_streams_stage1_train.py gives: the
streams taken here must not move the ones that file's check of the method itself has always had.
"""
import numpy as np
import pytest
import torch

import stream_cases as SC
from egoego_release_amd import stage1_data

pytestmark = pytest.mark.gpu

WINDOW, SEED, D = 16, 77, 512


def test_streams():
    g = np.random.default_rng(6)
    lens = [40, 18, 100, 33, 17]
    N, S = sum(lens), len(lens)
    up = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    pose, vels = up(g.normal(size=(N, 7)).astype(np.float32)), up(g.normal(size=(N, 6)).astype(np.float32))
    feats = up(g.normal(size=(N - S, D)).astype(np.float32))
    slam32, slam64 = up(g.normal(size=(N, 29)).astype(np.float32)), up(g.normal(size=(N, 3)))
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).cuda()  # (not late: a decoy of it is no offset table)
    ids = torch.tensor([4, 0, 2, 1, 3], dtype=torch.int32).cuda()
    draws = torch.tensor([9, 2 ** 40, 3, 11, 5], dtype=torch.int64).cuda()

    def call(p, v, f, s32, s64, i, d):
        tables = {"pose": p, "vels": v, "feats": f, "offsets": offsets, "slam32": s32, "slam_trans64": s64, "slam_offsets": offsets}
        b = stage1_data.head_batch(tables, i, d, WINDOW, SEED)
        return [b[k] for k in sorted(b)]

    true = [pose, vels, feats, slam32, slam64, ids, draws]
    call(*true)
    delay = SC.Delay().calibrate({"head batch": lambda: call(*true)})
    SC.check("egoego_s1_head_batch", SC.ENQUEUES, call, true, torch.cuda.Stream(), delay)
