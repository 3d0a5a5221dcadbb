"""CPU: the launch sequence of MistralDecoder.generate() (tools/decode_launch_trace.py: recording ops, a stand-in engine) against the
table recorded in tests/golden/decode_launch_trace.json -- per case the launch count, the prompt path and the SHA-256 of the whole trace
(op names, and per argument the scalar or buffer identity / offset / shape / strides / dtype).  Any reordered, added, dropped or
re-argumented launch of the decoder changes a hash; the fixture is a recorded result and is regenerated only by a change that means to
alter what the decoder launches."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "decode_launch_trace.py")
GOLDEN = os.path.join(ROOT, "tests", "golden", "decode_launch_trace.json")


def test_decoder_launch_sequence_matches_the_recorded_table():
    r = subprocess.run([sys.executable, TOOL, "--json"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, f"{len(bad)} of {len(want)} cases differ (python tools/decode_launch_trace.py --dump CASE shows a trace): {sorted(bad)}"


def test_recorded_table_holds_the_case_matrix():
    """dense x fuse_norm x rows x precision, MoE, and the prompt-path / sampling / logits / policy-switch cases; the launch counts of the
    default step at P = 3 prompt tokens on a 5-token prefix, 3 new tokens, 2 layers."""
    with open(GOLDEN) as f:
        t = json.load(f)
    for fuse in ("deferred", "deferred_mlp", "all", "qkv", "none"):
        for B in (1, 2, 3, 8, 9, 64):
            for p in ("bf16", "f16"):
                assert f"dense/{fuse}/B{B}/{p}" in t
    n = lambda k: (t[k]["launches"], t[k]["prefill"])
    assert [n(f"dense/deferred/B{B}/bf16") for B in (1, 3, 8, 9, 64)] == [(43, "rows"), (51, "rows"), (59, "rows"), (67, "rows"), (227, "rows")]
    assert [n(f"dense/none/B{B}/f16") for B in (1, 9, 64)] == [(45, "rows"), (69, "rows"), (229, "rows")]
    assert [n(f"dense/deferred_mlp/B{B}/bf16") for B in (1, 8, 9)] == [(64, "tokens"), (64, "tokens"), (74, "tokens")]
    assert [n(f"dense/all/B{B}/bf16") for B in (2, 3)] == [(64, "tokens"), (99, "tokens")]
    assert [n(f"dense/qkv/B{B}/bf16") for B in (2, 3)] == [(79, "tokens"), (99, "tokens")]
    assert n("dense/none/B1/bf16") == (99, "tokens")
    assert [n(f"moe/B{B}/{p}") for B in (1, 8) for p in ("bf16", "f16")] == [(114, "tokens"), (116, "tokens"), (394, "tokens"), (396, "tokens")]
    for k in ("no_chunk", "chunk_too_large", "sample", "return_logits", "no_past", "prefill_gemm"):
        assert any(c.startswith(k + "/") for c in t), k
    assert t["no_past/B3/bf16/engine_f16_operands"]["prefill"] == "encoder" and t["prefill_gemm/B3/f16/engine_bf16"]["prefill"] == "gemm"
