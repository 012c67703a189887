"""The shape-specialised instances of the fused pointwise backward (k_pw<M_BDC, .., FTW > 0, SP >> 8 != 0>, csrc/frost_pw.hip) against the generic instance.
frost_pw_conv_bwd_fused is called directly, twice on the same inputs and with round-to-nearest dc (FROST_SR=0: no random draws) -- once through the default dispatch,
once with FROST_PW_SPEC=0 (the switch is read by libfrost_hip.so at load: one child process per configuration, tools/pw_fused_digest.py).  The specialised
instances keep the generic tile-to-wave deal and its expressions, so dc and with it dx are the same bits; the weight-gradient sums are the same per workgroup and reach
memory through fp32 atomics whose order differs from run to run: the tolerance tests/test_gpu_paths.py uses for such sums (2e-5 of the norm).  The forward passes of these
layers are untouched by the switch's new reach: statistics tables and emitted bytes must be the same bits.
Each case runs three flavours of the call: (relu, accumulate 0), (the other relu, accumulate 1) and dx = NULL.  Sizes: 4 images of the layer's map at 56 x 56 and 8 at
28 x 28 (4 x 784 pixels are not a multiple of the 128-pixel tile the fused kernel needs): 98 / 49 tiles, one per workgroup; and more than 1024 tiles, where whatever
residency the launch gets (at most 4 workgroups on each of 256 CUs) some workgroups own two or more tiles and walk both LDS buffers."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (cin, cout, map, images, relu): Large @224's 24->72 and 24->144 (56 x 56 conv1), 56->168 (28 x 28 conv1 behind the squeeze cat), 144->40 and 168->40 (28 x 28 reduce convs)
SHAPES = [(24, 72, 56, 4, 1), (24, 144, 56, 4, 1), (56, 168, 28, 8, 1), (144, 40, 28, 8, 0), (168, 40, 28, 8, 0)]
CASES = SHAPES + [(24, 72, 56, 44, 0), (24, 144, 56, 44, 0), (56, 168, 28, 168, 0), (144, 40, 28, 168, 1), (168, 40, 28, 168, 1)]


def run(tmp, tag, case, env_extra, coef_from=None):
    out = os.path.join(tmp, f"{tag}.npz")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "pw_fused_digest.py"), out] + [str(v) for v in case] + ([coef_from] if coef_from else [])
    subprocess.run(cmd, check=True, env=dict(os.environ, FROST_SR="0", **env_extra), cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    return out


def relerr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def raw_sums(dwq, numel):
    """The raw weight-gradient sums: the kernels spread their flush atomics over copies at a stride of round_up(numel, 64)."""
    stride = (numel + 63) // 64 * 64
    return dwq.astype(np.float64).reshape(-1, stride)[:, :numel].sum(0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "_".join(str(v) for v in c))
def test_specialised_fused_backward_matches_generic_instance(case, tmp_path):
    cin, cout = case[0], case[1]
    assert (case[2] * case[2] * case[3]) % 128 == 0
    gen_path = run(str(tmp_path), "generic", case, {"FROST_PW_SPEC": "0"})
    new = np.load(run(str(tmp_path), "spec", case, {}, coef_from=gen_path))
    gen = np.load(gen_path)
    for tag in "abc":
        for k in ("y", "stats", "qy"):            # forward: statistics table, observer record, emitted bytes
            assert new[f"{tag}_{k}"].tobytes() == gen[f"{tag}_{k}"].tobytes(), (tag, k)
        assert new[f"{tag}_coef"].tobytes() == gen[f"{tag}_coef"].tobytes(), tag                      # identical inputs
        e_coef = relerr(new[f"{tag}_coef_after"], gen[f"{tag}_coef_after"])                           # S1 / S2 rows (the fused kernel only reads them)
        e_dw = relerr(raw_sums(new[f"{tag}_dwq"], cin * cout), raw_sums(gen[f"{tag}_dwq"], cin * cout))
        print(case, tag, "coef", e_coef, "dwq", e_dw, "|dwq|", float(np.linalg.norm(raw_sums(gen[f"{tag}_dwq"], cin * cout))))
        assert np.isfinite(gen[f"{tag}_dwq"]).all() and np.linalg.norm(gen[f"{tag}_dwq"]) > 0
        assert e_coef <= 2e-5 and e_dw <= 2e-5, (tag, e_coef, e_dw)
        if tag != "c":
            assert new[f"{tag}_dx"].tobytes() == gen[f"{tag}_dx"].tobytes(), (tag, "dx")
            assert np.any(gen[f"{tag}_dx"] != 0)
