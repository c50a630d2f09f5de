"""The stage-1 training entry points run on the caller's stream, and only there (include/egoego_hip.h, Conventions):
egoego_s1_train_forward, egoego_s1_headnet_loss and egoego_s1_train_backward under a side stream whose inputs arrive late, by the
method of tests/stream_cases.py.

A file of its own, collected behind tests/test_gpu_streams.py: every torch.cuda.Stream() a process takes moves the streams later
tests get on to other hardware queues, and test_gpu_streams.py's check of the method itself (a null-stream launch must overtake
the held side stream) needs the two on different queues — it is left with the streams it always had.
"""
from argparse import Namespace

import pytest
import torch

import stream_cases as SC
from egoego_release_amd import stage1, stage1_train
from egoego_release_amd.synthetic import make_stage1_train_batch

pytestmark = pytest.mark.gpu

WINDOW, LAYERS, W = 33, 2, 2


def test_streams():
    opt = Namespace(window=WINDOW, n_dec_layers=LAYERS, n_head=4, d_k=256, d_v=256, d_model=256, input_of_feats=True, dist_scale=10.0,
                    w_rotation=1.0, w_va=0.7, w_dist=0.4)
    m = stage1.HeadFormer(opt, torch.device("cuda")).cuda()
    eng = m.train_engine()
    ts = {n: p.detach() for n, p in m.named_parameters()}
    d = make_stage1_train_batch("headnet", W, WINDOW, seed=5, lengths=[WINDOW, 20])
    feats, pose, vels = d["of"].cuda(), d["head_pose"].cuda(), d["head_vels"].cuda()
    valid = d["seq_len"].cuda()
    up = torch.randn(W, WINDOW, 4, generator=torch.Generator().manual_seed(1)).cuda()

    def call(f, u):
        heads, saves = eng.forward(ts, f, valid, 0.1, 2)
        loss, d32, _ = stage1_train.headnet_loss(heads, WINDOW, pose, vels, opt.dist_scale, opt.w_rotation, opt.w_va, opt.w_dist)
        grads = eng.backward(ts, saves, u, W, 0.1, 2)
        return [heads, loss, d32] + [grads[k] for k in sorted(grads)]

    true = [feats, up]
    call(*true)
    delay = SC.Delay().calibrate({"stage-1 train step": lambda: call(*true)})
    SC.check("egoego_s1_train_forward + egoego_s1_headnet_loss + egoego_s1_train_backward", SC.ENQUEUES, call, true, torch.cuda.Stream(), delay)
