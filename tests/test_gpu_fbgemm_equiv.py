"""The path-equivalence tests of tests/test_gpu_paths.py and tests/test_gpu_block.py once more in per-channel + reduce_range mode (the 'fbgemm' qconfig):
tools/layer_digest.py / tools/block_digest.py with DIGEST_PER_CHANNEL=1 set `per_channel`, the per-channel observer buffers and index range 127.  The fast kernels
thread a per-channel `wscale` pointer and the record's upper index through the backward (the bf16 transposed pack carries wq * wscale[co] / scale, the depthwise
data-gradient kernels take `wscale` as an argument): a fast form that indexes it differently from its plain sibling shows here, under the per-tensor tests' own
assertions (the test functions and helpers are imported and called, not copied).  One case per kernel family, at the small batches of tests/test_gpu_fbgemm_paths.py.
Every digest run also records the C-ABI entries it launched; the fast entries a case is named for are asserted present in the fast run and absent from the plain one."""
import os

import pytest
import torch

import test_gpu_block as TB
import test_gpu_paths as TP

pytestmark = pytest.mark.gpu
GUARDED = ("frost_block_dw_bwd_c1", "frost_dw_bwd_fused_c1", "frost_sq_bwd_cat")          # fused forms the engine keeps off when conv1 is per-channel


@pytest.fixture
def calls(monkeypatch):
    """Every digest subprocess of the test runs with DIGEST_PER_CHANNEL=1 (the helpers build their environment from os.environ) and leaves its call log: {tag: entries}."""
    monkeypatch.setenv("DIGEST_PER_CHANNEL", "1")
    logs = {}

    def wrap(orig):
        def run(tmp, tag, case, env):
            path = env.get("DIGEST_CALLS") or os.path.join(tmp, f"calls_{tag}.txt")
            out = orig(tmp, tag, case, dict(env, DIGEST_CALLS=path))
            logs[tag] = open(path).read().split("\n")
            print(f"[per-channel digest {case} '{tag}'] entries: {' '.join(sorted(set(logs[tag])))}")
            return out
        return run
    monkeypatch.setattr(TP, "run", wrap(TP.run))
    monkeypatch.setattr(TB, "_digest", wrap(TB._digest))
    return logs


#        case                                   the fast entries it is named for (all of them switched off by test_gpu_paths.PLAIN)
FAMILY = [(("pw", 16, 96, 1, 1, 112, 2),        ("frost_pw_conv_bwd_fused",)),
          (("pw", 96, 24, 1, 1, 56, 2),         ("frost_pw_conv_bwd_fused",)),
          (("dw", 168, 168, 3, 1, 28, 3),       ("frost_dw_bwd_fused",)),
          (("dw", 144, 144, 5, 2, 56, 2),       ("frost_dw_bwd_fused",)),
          (("dw", 360, 360, 3, 1, 14, 7),       ("frost_block_dw_bwd", "frost_block_dw_bwd_reduce")),
          (("dw", 1440, 1440, 5, 1, 7, 5),      ("frost_block_dw_bwd", "frost_block_dw_bwd_reduce")),
          (("pw", 104, 624, 1, 1, 14, 6),       ("frost_pwc_conv_fwd_emit", "frost_pwc_conv_bwd", "frost_pw_dgrad_wide")),
          (("pw", 312, 80, 1, 1, 14, 3),        ("frost_pw_conv_fwd_keep", "frost_pw_ew", "frost_pw_dgrad_wide")),
          (("pw", 1440, 192, 1, 1, 7, 6),       ("frost_pw_conv_fwd_keep", "frost_pw_ew", "frost_pw_dgrad_wide"))]


@pytest.mark.parametrize("case,entries", FAMILY, ids=["_".join(str(v) for v in c) for c, _ in FAMILY])
def test_fast_paths_match_plain_paths_per_channel(calls, case, entries, tmp_path):
    err = None
    try:
        TP.test_fast_paths_match_plain_paths(case, tmp_path)
    except AssertionError as e:          # (the entries are checked first, so that a numeric mismatch on the WRONG path is reported as such; the mismatch itself is raised below)
        err = e
    assert "fast" in calls and "plain" in calls, err
    assert all(e in calls["fast"] for e in entries), (entries, sorted(set(calls["fast"])), err)
    assert not any(e in calls["plain"] for e in entries), (entries, sorted(set(calls["plain"])), err)
    if err is not None:
        raise err


@pytest.mark.parametrize("case", [("dw", 360, 360, 3, 1, 14, 7), ("dw", 1440, 1440, 5, 1, 7, 5)], ids=lambda c: "_".join(str(v) for v in c))
def test_fused_depthwise_backward_exact_without_stochastic_rounding_per_channel(calls, case, tmp_path):
    TP.test_fused_depthwise_backward_exact_without_stochastic_rounding(case, tmp_path)
    assert "frost_block_dw_bwd" in calls["fused"] and "frost_dw_dgrad" not in calls["fused"], sorted(set(calls["fused"]))
    assert "frost_dw_dgrad" in calls["sep"] and "frost_block_dw_bwd" not in calls["sep"], sorted(set(calls["sep"]))


@pytest.mark.parametrize("case", [("dw", 40, 40, 3, 1, 30, 5), ("dw", 168, 168, 3, 1, 28, 3), ("dw", 144, 144, 5, 2, 56, 2)], ids=lambda c: "_".join(str(v) for v in c))
@pytest.mark.parametrize("chunks", ["0", "3"])
def test_one_sweep_depthwise_backward_exact_without_stochastic_rounding_per_channel(calls, case, chunks, tmp_path):
    TP.test_one_sweep_depthwise_backward_exact_without_stochastic_rounding(case, chunks, tmp_path)
    assert "frost_dw_bwd_fused" in calls["one"] and "frost_dw_dgrad" in calls["sep"] and "frost_dw_bwd_fused" not in calls["sep"], (sorted(set(calls["one"])), sorted(set(calls["sep"])))


@pytest.mark.parametrize("case", [("dw", 40, 40, 3, 1, 30, 5), ("dw", 144, 144, 5, 2, 56, 2)], ids=lambda c: "_".join(str(v) for v in c))
def test_streaming_depthwise_passes_are_exact_per_channel(calls, case, tmp_path):
    """(The strip-streaming passes are chosen INSIDE frost_dw_conv_fwd_fin / frost_dw_conv_fwd / frost_dw_conv_bwd by frost_dws_ok: the call log shows those entries in both runs.)"""
    TP.test_streaming_depthwise_passes_are_exact(case, tmp_path)
    assert "frost_dw_conv_fwd_fin" in calls["new"] and calls["new"] == calls["old"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()


@pytest.mark.parametrize("case", [(104, 624, 14, 5, 96, 3), (120, 360, 14, 3, 96, 33), (240, 1440, 7, 5, 192, 5)], ids=lambda c: "_".join(str(v) for v in c))
def test_block_kernels_bit_identical_to_layer_launches_per_channel(built, case, monkeypatch):
    """In process (this test has no digest): test_gpu_block._build's layers switched to per-channel + reduce_range before the first step."""
    from frostnet_amd import _lib as L
    build = TB._build

    def build_pc(*a):
        E, l1, l2, l3, qx = build(*a)
        for l in (l1, l2, l3):
            l.per_channel = True
            l.wmin, l.wmax = torch.full((l.cout,), float("inf"), device="cuda"), torch.full((l.cout,), float("-inf"), device="cuda")
            l.qy[L.Q_QMAX] = 127.0
        qx[L.Q_QMAX] = 127.0
        E.act_qmax = 127
        return E, l1, l2, l3, qx
    monkeypatch.setattr(TB, "_build", build_pc)
    L.CALL_LOG = []
    try:
        TB.test_block_kernels_bit_identical_to_layer_launches(case)
        log = list(L.CALL_LOG)
    finally:
        L.CALL_LOG = None
    print(f"[per-channel block {case}] entries: {' '.join(sorted(set(log)))}")
    assert ("frost_block_expand_dw_stats" in log or "frost_block_dw_stats" in log) and "frost_block_dw_reduce" in log, sorted(set(log))


@pytest.mark.parametrize("case", TB.BWD_CASES[:2], ids=lambda c: "_".join(str(v) for v in c))
def test_block_backward_without_stochastic_rounding_per_channel(calls, case, tmp_path):
    TB.test_block_backward_without_stochastic_rounding(case, tmp_path)
    blk, lay = calls["blk"], calls["lay"]
    assert "frost_block_dw_bwd" in blk and "frost_block_dw_bwd_reduce" in blk and "frost_block_dw_reduce" in blk, sorted(set(blk))
    assert not any(e.startswith("frost_block_") for e in lay), sorted(set(lay))


@pytest.mark.parametrize("case", [(104, 624, 14, 5, 96, 3), (120, 360, 14, 3, 96, 7), (16, 96, 112, 3, 24, 2, 2)], ids=lambda c: "_".join(str(v) for v in c))
def test_guarded_fused_forms_stay_off_per_channel(calls, case, tmp_path):
    """With the defaults (conv1 folds ON) a per-channel conv1 keeps the engine on the unfused siblings: frost_block_dw_bwd (not _c1) at 14 x 14, frost_dw_bwd_fused (not _c1)
    on the stride-2 one-sweep layer, and conv1 runs a reduce pass of its own.  The same digest per-tensor DOES take the folded form (asserted: the guard is what differs)."""
    TB._digest(str(tmp_path), "pc", case, {})
    TB._digest(str(tmp_path), "pt", case, {"DIGEST_PER_CHANNEL": "0"})
    pc, pt = calls["pc"], calls["pt"]
    sibling = "frost_dw_bwd_fused" if len(case) > 6 else "frost_block_dw_bwd"
    assert not any(g in pc for g in GUARDED) and sibling in pc, sorted(set(pc))
    assert sibling + "_c1" in pt and sibling not in pt, sorted(set(pt))
    reduce_passes = lambda log: log.count("frost_pw_conv_bwd") + log.count("frost_pwc_conv_bwd")
    assert reduce_passes(pc) == reduce_passes(pt) + 1, (sorted(pc), sorted(pt))
