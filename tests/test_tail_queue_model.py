"""The counted vector-memory waits of the head-major int8 fc (tail_fused.h DirectGemm::run_heads) are guarded by a constexpr replay
of the wave's memory queue (FcQueueModel) that the kernel static_asserts on.  Compile-only (no GPU): the model accepts the tables
of every form the library builds or can be configured to, and it does reject a count that is off by one in either direction —
so a miscounted wait stops the build instead of reaching a device."""
import os
import subprocess

from egoego_release_amd import build as B

SRC = r"""
#include "tail_fused.h"
// <feature tiles per pass, token tiles, ring slots, DMA pieces per wave, int8, third-slice form, feature passes, heads>
template <int FT, int TT, int RING, bool WLO0, int FP, int NH>
constexpr bool tight() {
    using G = DirectGemm<FT, TT, RING, false, true, 4, WLO0>;
    using M = FcQueueModel<FT, TT, RING, G::DMA_PIECES, true, WLO0, FP, NH>;
    constexpr int n = G::template heads_dma_wait<FP>();
    // the shipped count is tight; one more would let an awaited piece stay in flight, one fewer would drain a prefetch (when below the counter's cap)
    // (a single head requests no further chunk: nothing depends on the count)
    return M::check(n) == 0 && (NH == 1 || ((n >= 63 || M::check(n + 1) != 0) && (n == 0 || M::check(n - 1) != 0)));
}
static_assert(tight<2, 1, 4, false, 2, 4>() && tight<2, 1, 4, true, 2, 4>(), "the two-workgroups-per-CU tail, with and without the third weight slice");
static_assert(tight<2, 1, 4, false, 2, 1>() && tight<2, 1, 4, false, 2, 2>() && tight<2, 1, 4, false, 2, 16>(), "1, 2 and 16 heads");
static_assert(tight<2, 1, 8, false, 2, 4>() && tight<2, 2, 4, false, 2, 4>() && tight<2, 2, 8, true, 2, 4>(), "the deep-ring and the 64-token configurations");
// the numbers themselves for the shipped form: 7 + 8 k-steps of 4 weight fragments are issued behind a chunk's pieces
static_assert(FcQueueModel<2, 1, 4, 4, true, false, 2, 4>::check(60) == 0 && FcQueueModel<2, 1, 4, 4, true, false, 2, 4>::check(56) != 0, "");
"""


def test_counted_waits_of_the_head_major_fc_match_its_issue_order(tmp_path):
    f = tmp_path / "queue_model.hip"
    f.write_text(SRC)
    r = subprocess.run([B._hipcc(), "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", B.CSRC, str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_a_miscounted_wait_does_not_compile(tmp_path):
    f = tmp_path / "queue_model_bad.hip"
    f.write_text('#include "tail_fused.h"\nstatic_assert(FcQueueModel<2, 1, 4, 4, true, false, 2, 4>::check(61) == 0, "miscount");\n')
    r = subprocess.run([B._hipcc(), "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", B.CSRC, str(f)], capture_output=True, text=True)
    assert r.returncode != 0 and "miscount" in r.stderr
