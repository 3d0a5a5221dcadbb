"""CPU: the launch sequences of the encoder engine and the training engines (tools/encoder_launch_trace.py: recording ops, the real
engines on small CPU tensors) against the table recorded in tests/golden/encoder_launch_trace.json -- per case the launch count and the
SHA-256 of the whole trace (op names; per argument the scalar or buffer identity / offset / shape / strides / dtype and the values of
small integer tensors; what every call returned or raised).  Any reordered, added, dropped or re-argumented launch, a changed batch
geometry or a changed aliasing of a result changes a hash; the fixture is a recorded result and is regenerated only by a change that
means to alter what the engines launch."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "encoder_launch_trace.py")
GOLDEN = os.path.join(ROOT, "tests", "golden", "encoder_launch_trace.json")
POLICIES = ("bf16", "fp32_residual", "f16_operands", "f16_stream")


def test_engine_launch_sequences_match_the_recorded_table():
    r = subprocess.run([sys.executable, TOOL, "--json"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, f"{len(bad)} of {len(want)} cases differ (python tools/encoder_launch_trace.py --dump CASE shows a trace): {sorted(bad)}"


def test_recorded_table_holds_the_case_matrix():
    """encoder forward x policy x attention x variant, encode_pooled x policy x packed x batch, forward_on_cache, the MoE engine, the
    training engines (no-grad policies, padded / packed, save, causal, backward with and without recompute, a parameter update between
    fp16 calls) and the refused combinations; launch counts of the plain cases at 2 layers (two calls where a case makes two)."""
    with open(GOLDEN) as f:
        t = json.load(f)
    n = lambda k: t[k]["launches"]
    for pol in POLICIES:
        for mode in ("bidir", "causal", "window"):
            for v in ("plain", "borrow", "return_kv_bf16", "return_kv_none", "inputs_embeds", "layer_range"):
                assert f"encoder/forward/{pol}/{mode}/{v}" in t
            assert n(f"encoder/forward/{pol}/{mode}/plain") == 17
        for packed in (None, True, False):
            for kind in ("ragged", "full", "holes"):
                assert f"encoder/encode_pooled/{pol}/packed_{packed}/{kind}" in t
        assert n(f"encoder/encode_pooled/{pol}/packed_None/ragged") == 2 * 17 and n(f"encoder/encode_pooled/{pol}/packed_None/holes") == 2 * 18
        assert n(f"encoder/forward_on_cache/{pol}/final_norm_True") == 18 and n(f"encoder/forward_on_cache/{pol}/final_norm_False") == 17
    assert "encoder/successive_calls_and_policy_switch" in t
    for pol in ("bf16", "f16_operands"):
        assert n(f"moe/forward/{pol}") == 21 and f"moe/encode_pooled/{pol}/packed_None" in t
        for layout, dense, moe in (("padded", 17, 21), ("packed", 16, 20)):
            for save in (False, True):
                assert n(f"train/forward/{pol}/{layout}/save_{save}/causal_False") == dense
                assert n(f"mixtral/forward/{pol}/{layout}/save_{save}/causal_False") == moe
    for pol in ("bf16", "f16_operands", "f16_stream"):
        assert f"train/forward/{pol}/packed/save_False/causal_True" in t and f"train/forward_pooled/{pol}" in t
    for name in ("train", "mixtral"):
        for rc in (False, True):
            assert f"{name}/forward_backward/recompute_{rc}/packed" in t and f"{name}/forward_backward_pooled/recompute_{rc}" in t
    assert "train/param_update_between_calls/f16_operands" in t and "mixtral/param_update_between_calls/f16_operands" in t
    refused = [k for k in t if k.startswith("refused/")]
    assert len(refused) == 8
    # (a policy ASSIGNED to a sparse-MoE engine, past set_precision's refusal, is refused by the MoE block itself, 7 launches in)
    assert [n(k) for k in sorted(refused)] == [0, 0, 0, 0, 0, 7, 0, 0]
