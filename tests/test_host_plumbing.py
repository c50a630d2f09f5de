"""The host plumbing the satellite modules share (csrc/host_util.h, _engine.py, _lib's check factory), the parts that need no
GPU: every module keeps an error slot of its own, per thread; the check functions carry the module's prefix; the engines refuse a
CPU device by name.  The calls below fail on their arguments before they touch a device."""
import ctypes as C
import threading

import pytest

from egoego_release_amd import _lib, body, stage1
from egoego_release_amd.synthetic import Stage1Config

E_INVALID = -1  # EGOEGO_E_INVALID (include/egoego_hip.h)


def _s1_create(lib, kind):
    cfg = _lib.S1Config(kind, 512, 256, 4, 1, 256, 256, 31)
    out = C.c_void_p()
    return lib.egoego_s1_ctx_create(C.byref(cfg), 0, C.byref(out))


def _fail_all(lib):
    """One failing call per module -> {module: (return code, its last error)}, the errors read after all four calls."""
    out = C.c_void_p()
    rc = {"flow": lib.egoego_flow_ctx_create(0, -1, C.byref(out)),
          "body": lib.egoego_body_ctx_create(0, -1, C.byref(out)),
          "s1": _s1_create(lib, 7),
          "eval": lib.egoego_eval_shift_xy(None, 1, 1, 0, None)}
    return {k: (rc[k], getattr(lib, f"egoego_{k}_last_error")().decode()) for k in rc}


def test_every_module_keeps_its_own_error_slot():
    lib = _lib.load()
    before = lib.egoego_last_error()
    got = _fail_all(lib)
    assert got == {"flow": (E_INVALID, "chunk_frames -1: 0..4096 accepted"),
                   "body": (E_INVALID, "chunk_frames -1: 0..65536 accepted"),
                   "s1": (E_INVALID, "unknown kind 7"),
                   "eval": (E_INVALID, "NULL argument")}
    assert lib.egoego_last_error() == before  # the denoiser's slot is not theirs


def test_the_error_slot_is_per_thread():
    lib = _lib.load()
    assert _s1_create(lib, 7) == E_INVALID
    seen = {}

    def other():
        seen["rc"] = _s1_create(lib, 9)
        seen["err"] = lib.egoego_s1_last_error().decode()

    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen == {"rc": E_INVALID, "err": "unknown kind 9"}
    assert lib.egoego_s1_last_error().decode() == "unknown kind 7"


@pytest.mark.parametrize("name,prefix,module", [("check_s1", "stage-1", "s1"), ("check_flow", "flow-CNN", "flow"),
                                                ("check_body", "body-model", "body"), ("check_eval", "evaluation", "eval")])
def test_check_raises_with_the_modules_prefix_code_and_text(name, prefix, module):
    rc, text = _fail_all(_lib.load())[module]
    check = getattr(_lib, name)
    check(0)
    with pytest.raises(_lib.EgoEgoHipError) as e:
        check(rc)
    assert str(e.value) == f"libegoego_hip {prefix} error {rc}: {text}"
    if module == "s1":
        assert str(e.value) == "libegoego_hip stage-1 error -1: unknown kind 7"


@pytest.mark.parametrize("make,noun", [(lambda: stage1.Stage1Engine(Stage1Config("headnet", 31, 1), "cpu"), "stage 1"),
                                       (lambda: stage1.FlowCNNEngine("cpu"), "the flow CNN"),
                                       (lambda: body.BodyEngine("cpu"), "the body model")])
def test_an_engine_on_a_cpu_device_raises_with_its_modules_noun(make, noun):
    with pytest.raises(_lib.EgoEgoHipError) as e:
        make()
    assert str(e.value) == f"{noun} needs a cuda (ROCm) device; there is no CPU path"
