"""The workspace audit of DESIGN.md 4a, held to the sources.

Every GPU entry point works in a caller-supplied workspace whose contents on entry must not matter (include/egoego_hip.h,
Conventions).  REGIONS below names every region the sources carve — the pointer members of `struct Workspace` (egoego_hip.hip) and
the regions of the satellite layouts (stage1.hip, flow_cnn.hip, body_model.hip, egoego_win_stats) — with the kernel that writes it in
every call, whether a call may read it before that write ("stale": as DATA of rows that are never stored — never as an index), and
whether it persists between calls.  A region added to the sources without an entry, or an entry whose region is gone, fails here;
the GPU side of the same contract is tests/test_gpu_workspace.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "egoego_release_amd", "csrc")


def R(writer, stale=None, persistent=False):
    """writer: what writes the region in every call that reads it; stale: None, or why what a call reads there before writing it
    cannot reach a stored result; persistent: survives between calls by design (the caller establishes it, see the header)."""
    return {"writer": writer, "stale": stale, "persistent": persistent}


PAD_ROWS = "rows Mvalid..Mp-1 only: a token is one MFMA column and one lane of every reduction; EpiOut stores b < B, the monitor " \
           "counts rows < outlier_rows, the next projections skip m0 >= Mvalid"
REGIONS = {
    "stage2": {
        "state": R("k_state_init (loop calls); embed / out epilogues publish out_step / embed_step",
                   stale="ln_max only: accumulated by atomicMax, read by egoego_outlier_stats alone", persistent=True),
        "step_ts": R("hipMemcpyAsync in ddim_loop_impl, entries 0..n-1"),
        "step_tab": R("hipMemcpyAsync in ddim_loop_impl, entries 0..n-1"),
        "t_idx": R("k_convert_t, entries 0..B-1"),
        "row_mask": R("k_pack_row_mask, all Mp rows (nullptr reaches the kernels without a mask)"),
        "xall": R("k_pack_pose, all Mp rows x KE columns; EpiOut rewrites the valid rows"),
        "hA": R("embed epilogue, all Mp rows; LayerNorm-2 of every layer"),
        "hB": R("LayerNorm-1 of every layer, all rows of its blocks", stale=PAD_ROWS),
        "F": R("FFN-1 epilogue, all rows of its blocks", stale=PAD_ROWS),
        "Q": R("EpiQK rows < Mvalid / qkv_i8q_kernel queries 0..Lr-1 / attn_proj*_i8_kernel whole images",
               stale="int8 images, queries Lr..Lp-1: computed, never stored (active)"),
        "K": R("EpiQK rows < Mvalid / qkv_i8q_kernel keys 0..Lr-1 / attn_proj*_i8_kernel whole images",
               stale="int8 images, keys Lr..Lp-1: their scores are replaced by -inf by a select on the key index"),
        "V": R("EpiV rows < Mvalid / qkv_i8q_kernel keys 0..Lr-1 / attn_proj*_i8_kernel whole images and column scales",
               stale="int8 images, keys Lr..Lp-1: integer bytes times a probability quantised to integer 0"),
        "O": R("attention kernels, rows < Mvalid", stale=PAD_ROWS),
        "hA8": R("embed epilogue, all Mp rows; LayerNorm-2 of every layer"),
        "hA_scale": R("embed epilogue, all Mp rows; LayerNorm-2 of every layer"),
        "hB8": R("LayerNorm-1 of every layer, all rows of its blocks", stale=PAD_ROWS),
        "F8": R("FFN-1 epilogue, all rows of its blocks", stale=PAD_ROWS),
        "hB_scale": R("LayerNorm-1 of every layer, all rows of its blocks", stale=PAD_ROWS),
        "F_scale": R("FFN-1 epilogue, all rows of its blocks", stale=PAD_ROWS),
        "O8": R("int8 attention kernels, rows < Mvalid", stale=PAD_ROWS),
        "O_scale": R("int8 attention kernels, rows < Mvalid", stale=PAD_ROWS),
        "att_img": R("alias of Q and K: attn_proj*_i8_kernel, the three whole images of every (window, head)"),
        "sq8": R("qkv_i8q_kernel / attn_proj*_i8_kernel, queries 0..Lr-1", stale="queries Lr..Lp-1: never stored (active)"),
        "sk8": R("qkv_i8q_kernel / attn_proj*_i8_kernel, keys 0..Lr-1", stale="keys Lr..Lp-1: masked by a select before the maximum"),
        "sv8": R("hipMemsetAsync in pack_inputs when Lr != Lp, then qkv_i8q_kernel keys 0..Lr-1"),
    },
    "stage1": {
        "X": R("s1_embed_kernel, all W * Lp rows; s1_tail_kernel in place"),
        "QKV": R("s1_linear_kernel, all rows"),
        "O": R("s1_attn_kernel, all rows"),
        "H1": R("alias of QKV: s1_linear_kernel (head layer 0), every row of the launch"),
        "H3": R("alias of QKV: s1_linear_kernel (head layer 2), every row of the launch"),
        "H2": R("alias of O: s1_linear_kernel (head layer 1), every row of the launch"),
    },
    "flow": {
        "buf": R("flow_conv_kernel / flow_maxpool_kernel: every output of the chunk's F frames before a launch reads it"),
        "pooled": R("flow_avgpool_kernel, F x 512"),
    },
    "body": {
        "v_shaped": R("body_shape_kernel, every entry"),
        "J": R("body_shape_kernel, every entry"),
        "A": R("body_frame_kernel, frames < F (body_skin_kernel reads frames < F)"),
        "fhi": R("body_frame_kernel, rows < F, K padding zeroed",
                 stale="rows F..32 * ceil(F / 32) - 1: the frame side of the MFMAs, one row per output; rows >= F are not stored"),
        "flo": R("body_frame_kernel, rows < F, K padding zeroed",
                 stale="rows F..32 * ceil(F / 32) - 1: the frame side of the MFMAs, one row per output; rows >= F are not stored"),
    },
    "win_stats": {
        "part": R("win_minmax_kernel: every workgroup writes its whole row (+-inf without a frame) before the fold"),
    },
}


def _src(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def _function_body(src, head):
    """The text of the function whose definition starts with `head`, up to the first line that holds only its closing brace."""
    i = src.index(head)
    return src[i:src.index("\n}", i)]


def stage2_regions(src=None):
    """Pointer members of `struct Workspace` in egoego_hip.hip, in declaration order."""
    src = _src("egoego_hip.hip") if src is None else src
    body = re.search(r"struct Workspace \{(.*?)\n\};", src, re.S).group(1)
    names = []
    for decl in body.split(";"):
        if "*" in decl:
            names += re.findall(r"\*\s*(\w+)", decl)
    return names


def stage1_regions():
    body = _function_body(_src("stage1.hip"), "int egoego_s1_encode(")
    return re.findall(r"\bfloat\* (\w+) = ", body)


def flow_regions():
    body = _function_body(_src("flow_cnn.hip"), "int egoego_flow_features(")
    body = body[body.index(") {"):body.index("for (int f0")]  # the carving: behind the signature, before the chunk loop
    names = re.findall(r"\bfloat\* (\w+)", body)
    assert names[0] == "ws"  # the base pointer itself
    return names[1:]


def body_regions():
    m = re.search(r"struct WsLayout \{\s*size_t ([^;]*);", _src("body_model.hip"))
    names = [n.strip() for n in m.group(1).split(",")]
    assert names[-1] == "total"
    return names[:-1]


def win_stats_regions():
    body = _function_body(_src("motion_windows.hip"), "int egoego_win_stats(")
    uses = re.findall(r"\((?:const )?float\*\)workspace", body)
    assert len(uses) == 2, uses  # the partials: win_minmax_kernel's out, win_minmax_fold_kernel's part
    m = re.search(r"void win_minmax_fold_kernel\(const float\* (\w+),", _src("motion_windows.h"))
    return [m.group(1)]


PARSED = {"stage2": stage2_regions, "stage1": stage1_regions, "flow": flow_regions, "body": body_regions, "win_stats": win_stats_regions}


def test_the_parsers_find_the_layouts():
    """(guards the regexes: a source reshaped so that a parser finds nothing must not pass as 'no regions')"""
    got = {k: f() for k, f in PARSED.items()}
    assert len(got["stage2"]) >= 25 and got["stage2"][0] == "state" and "sv8" in got["stage2"], got["stage2"]
    assert got["stage1"][:3] == ["X", "QKV", "O"], got["stage1"]
    assert got["flow"] == ["buf", "pooled"], got["flow"]
    assert got["body"][0] == "v_shaped" and len(got["body"]) == 5, got["body"]
    assert got["win_stats"] == ["part"]


def test_every_workspace_region_is_audited_and_every_entry_exists():
    assert set(PARSED) == set(REGIONS)
    for mod, parse in PARSED.items():
        src, table = parse(), REGIONS[mod]
        assert len(src) == len(set(src)), (mod, src)
        assert set(src) == set(table), {"module": mod, "carved in the source, not in REGIONS": sorted(set(src) - set(table)),
                                       "in REGIONS, gone from the source": sorted(set(table) - set(src))}
        for name, r in table.items():
            assert set(r) == {"writer", "stale", "persistent"} and r["writer"], (mod, name)
            assert isinstance(r["persistent"], bool) and (r["stale"] is None or r["stale"]), (mod, name)


def test_a_region_without_an_entry_fails():
    """A member added to struct Workspace is found by the parser (so the test above fails until it has an entry), and an entry
    deleted from REGIONS leaves a carved region unaudited."""
    src = _src("egoego_hip.hip")
    grown = src.replace("struct Workspace {", "struct Workspace {\n    float* new_scratch;\n    int8_t *more8, *more9;", 1)
    assert set(stage2_regions(grown)) - set(REGIONS["stage2"]) == {"new_scratch", "more8", "more9"}
    for name in REGIONS["stage2"]:
        assert set(stage2_regions()) - (set(REGIONS["stage2"]) - {name}) == {name}


def test_carve_places_every_region_and_nothing_else():
    """carve() assigns every pointer member of struct Workspace, each from take() (att_img: the alias of Q)."""
    body = _function_body(_src("egoego_hip.hip"), "static void carve(")
    placed = [n for n in re.findall(r"\bw\.(\w+) = \(", body) if not n.endswith("_plane")]  # (the plane strides are sizes)
    assert sorted(placed) == sorted(stage2_regions()), sorted(set(placed) ^ set(stage2_regions()))
    for name in placed:
        rhs = re.search(rf"\bw\.{name} = ([^;]*);", body).group(1)
        assert "take(" in rhs or name == "att_img", (name, rhs)


def test_the_outlier_monitor_is_the_only_persistent_region():
    """Persistent state is what a caller must establish: today StepState::ln_max alone, cleared through egoego_outlier_stats —
    named in the header, INTEGRATION.md and DESIGN.md.  k_state_init, which arms the rest of the step state in every loop call,
    must not touch it."""
    persistent = [(m, n) for m, t in REGIONS.items() for n, r in t.items() if r["persistent"]]
    assert persistent == [("stage2", "state")]
    init = _function_body(_src("pointwise.h"), "__global__ void k_state_init(")
    fields = re.search(r"struct StepState \{(.*?)\n\};", _src("common.h"), re.S).group(1)
    members = [re.findall(r"(\w+)(?:\[\d+\])?$", d.strip())[0] for d in fields.split(";") if d.strip()]
    assert members[-1] == "ln_max" and len(members) == 12, members
    assert set(re.findall(r"st->(\w+) =", init)) == set(members) - {"ln_max"}  # every index / pointer of the state, not the monitor
    stats = _function_body(_src("egoego_hip.hip"), "int egoego_outlier_stats(")
    assert "hipMemsetAsync(w.state->ln_max, 0" in stats
    header = open(os.path.join(ROOT, "include", "egoego_hip.h")).read()
    for doc in (header, open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        flat = " ".join(doc.replace(" *", " ").split())
        assert "irrelevant to every result" in flat and "outlier monitor" in flat, "the workspace contract is stated"
        assert re.search(r"egoego_outlier_stats\(ctx, B, T, ws, bytes, NULL, 0, 1, stream\)", flat)


def test_the_sv8_clear_is_in_place():
    """The one region where 'meets a probability of 0' was not enough (0 x NaN): keys Lr..Lp-1 exist in the attention images only
    and their V scales are cleared in every call, outside the captured step."""
    pack = _function_body(_src("egoego_hip.hip"), "static int pack_inputs(")
    assert re.search(r"if \(g\.Lr != g\.Lp\)\s*HIP_TRY\(hipMemsetAsync\(w\.sv8, 0, sizeof\(float\) \* \(size_t\)g\.B \* c->H \* g\.Lp, s\)\);", pack)


def test_design_md_lists_every_region():
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = doc[doc.index("### 4a. The workspaces"):doc.index("## 5. Kernels")]
    for mod, table in REGIONS.items():
        for name, r in table.items():
            assert re.search(rf"`(?:state->)?{re.escape(name)}(?:\[[^\]]*\))?`", sec), (mod, name)
    # rows that own up to a stale read are marked, the others say "no"
    n_yes = len(re.findall(r"\*\*yes", sec))
    assert n_yes == 3 and "**persistent**" in sec
