"""egoego_s1_gravity_batch runs on the caller's stream, and only there (include/egoego_hip.h, Conventions): the batch
build under a side stream whose inputs (the packed poses, the sequence ids, the draw ids) arrive late, by the method of
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

WINDOW, SEED = 16, 77


def test_streams():
    g = np.random.default_rng(5)
    lens = [40, 17, 100, 33, 18]
    pose = torch.from_numpy(g.normal(size=(sum(lens), 7)).astype(np.float32)).cuda()
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).cuda()  # (not late: a decoy of it is no offset table)
    ids = torch.tensor([4, 0, 2, 1, 3], dtype=torch.int32).cuda()
    draws = torch.tensor([9, 2 ** 40, 3, 11, 5], dtype=torch.int64).cuda()

    def call(p, i, d):
        b = stage1_data.gravity_batch(p, offsets, i, d, WINDOW, SEED)
        return [b[k] for k in sorted(b)]

    true = [pose, ids, draws]
    call(*true)
    delay = SC.Delay().calibrate({"gravity batch": lambda: call(*true)})
    SC.check("egoego_s1_gravity_batch", SC.ENQUEUES, call, true, torch.cuda.Stream(), delay)
