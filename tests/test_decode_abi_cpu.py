"""CPU: the refusals of the decode entry points (csrc/decode.hip, decode_gemm.hip, sample.hip) are ABI.
tests/golden/decode_abi_refusals.json holds, for a deterministic table of calls with one rule broken (and a few with two, which pin the
ORDER of the rules), the return code and the grit_last_error_string() of the library the table was recorded from; the library under test
must answer every call of the table with the same code and the same message, byte for byte.

Every call of the table is refused (GRIT_E_BADARG, GRIT_E_UNSUPPORTED) or is a no-op (GRIT_OK for zero rows; the sizes and zeros of
grit_attn_decode_workspace_floats, which has no error channel): none gets as far as a launch.  Every call passes HOST pointers, so the
module skips itself where a device is present: there a validation that lets one through would launch a kernel on them; without a device
such a call ends in GRIT_E_LAUNCH and fails the comparison.

Recording (from the revision whose behaviour is to be pinned; --source names that revision's three .hip files, whose GRIT_REQUIRE
messages -- all that a default build can reach -- must be hit by the table):
    GRIT_HIP_LIB=<that revision's libgritlm_hip.so> python tests/test_decode_abi_cpu.py --record --source decode.hip decode_gemm.hip sample.hip"""
import ctypes
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from gritlm_amd import _lib  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "decode_abi_refusals.json")
RECORDED_CODES = (_lib.GRIT_OK, _lib.GRIT_E_BADARG, _lib.GRIT_E_UNSUPPORTED)
# reached only through the group-per-workgroup launch of grit_attn_decode*, which no default build takes for a group size it lacks
UNREACHABLE = ("query heads per kv head (1, 2, 4 or 8 are built)",)
N_REQUIRES = 47     # distinct reachable GRIT_REQUIRE messages of the three files at the recorded revision

_buf = (ctypes.c_char * 4096)()
P = (ctypes.addressof(_buf) + 15) & ~15          # a 16-byte-aligned host address stands in for every pointer
INF, NAN = float("inf"), float("nan")

PROJ = ["x", "W", "out", "B", "N", "K", "ldx", "ldw", "ldo", "epilogue", "residual", "ldr", "stream"]
PROJ_F16 = PROJ[:-1] + ["out16", "ldo16", "stream"]
NORM = ["x", "ln_weight", "eps", "W", "out", "B", "N", "K", "ldx", "ldw", "ldo", "epilogue", "stream"]
EXPERT = ["x", "W", "out", "expert", "w_expert_stride", "E", "B", "N", "K", "ldx", "ldw", "ldo", "epilogue", "stream"]
ROPE_APPEND = ["qkv", "cos_tab", "sin_tab", "cache_k", "cache_v", "lens", "B", "nq", "nkv", "d", "Lmax", "qkv_stride", "stream"]
ROPE_APPEND_ROWS = ROPE_APPEND[:6] + ["cache_row"] + ROPE_APPEND[6:-1] + ["f16", "stream"]
KV_APPEND = ["qkv", "cache_k", "cache_v", "lens", "B", "nq", "nkv", "d", "Lmax", "qkv_stride", "stream"]
WORKSPACE = ["B", "nq", "nkv", "Lmax"]
ATTN = ["q", "cache_k", "cache_v", "lens", "out", "workspace", "B", "nq", "nkv", "d", "Lmax", "q_stride", "out_stride", "scale", "stream"]
ATTN_ROWS = ATTN[:4] + ["cache_row"] + ATTN[4:-1] + ["f16", "stream"]
ATTN_ROPE = ["q", "cos_tab", "sin_tab", "cache_k", "cache_v", "lens", "out", "workspace", "B", "nq", "nkv", "d", "Lmax", "q_stride", "out_stride",
             "scale", "stream"]
ARGMAX = ["logits", "ld", "V", "next", "lens", "history", "hist_stride", "step", "B", "stream"]
SAMPLE = ARGMAX + ["temperature", "top_k", "top_p", "keys"]
COMBINE = ["h", "h16", "y", "weights", "B", "H", "stream"]

# valid calls (they would launch): every rule below changes one of them
_PROJ = dict(x=P, W=P, out=P, B=2, N=64, K=64, ldx=64, ldw=64, ldo=64, epilogue=0, residual=None, ldr=0, out16=None, ldo16=0, ln_weight=P,
             eps=1e-5, stream=None)
_EXPERT = dict(_PROJ, expert=P, w_expert_stride=64 * 64, E=5)
_ATTN = dict(q=P, qkv=P, cos_tab=P, sin_tab=P, cache_k=P, cache_v=P, lens=P, cache_row=P, out=P, workspace=P, B=2, nq=4, nkv=2, d=128, Lmax=256,
             q_stride=1024, qkv_stride=1024, out_stride=512, scale=0.088, f16=0, stream=None)
_TOKEN = dict(logits=P, ld=1008, V=1001, next=P, lens=None, history=None, hist_stride=0, step=None, B=2, stream=None, temperature=1.0, top_k=0,
              top_p=1.0, keys=P)
_COMBINE = dict(h=P, h16=P, y=P, weights=P, B=2, H=64, stream=None)


def _nulls(names):
    return {f"{n}=null": {n: None} for n in names}


def _misaligned(names):
    return {f"{n} misaligned": {n: P + 4} for n in names}


def _proj_rules(gemm, f16, norm):
    """the GEMV (1..8 rows, K % 8) and the MFMA row GEMM (1..64 rows, K % 64, N % 16); norm: the fused-norm entry points"""
    r = _nulls(["x", "W", "out"] + (["ln_weight"] if norm else []))
    r.update(_misaligned(["x", "W"] + (["ln_weight"] if norm else [])))
    r.update({"B=0": dict(B=0), "B<0": dict(B=-1), "B too large": dict(B=65 if gemm else 9), "N=0": dict(N=0), "N<0": dict(N=-64),
              "K=0": dict(K=0), "K<0": dict(K=-64), "K % 8": dict(K=60), "ldx short": dict(ldx=56), "ldx % 8": dict(ldx=68),
              "ldw short": dict(ldw=56), "ldw % 8": dict(ldw=68), "ldo < N": dict(ldo=32),
              "SWIGLU N % 32": dict(epilogue=2, N=48), "SWIGLU ldo < N/2": dict(epilogue=2, ldo=16),
              "unknown epilogue": dict(epilogue=7), "epilogue<0": dict(epilogue=-1), "RESIDUAL, residual=null": dict(epilogue=1)})
    if gemm:
        r.update({"K % 64": dict(K=96, ldx=96, ldw=96), "N % 16": dict(N=24, ldo=24)})
    if not norm:
        r.update({"RESIDUAL ldr < N": dict(epilogue=1, residual=P, ldr=32), "RESIDUAL ldo < N": dict(epilogue=1, residual=P, ldr=64, ldo=32)})
        if f16:
            r.update({"out16 with STORE": dict(out16=P, ldo16=64), "out16 with SWIGLU": dict(out16=P, ldo16=64, epilogue=2),
                      "RESIDUAL ldo16 < N": dict(epilogue=1, residual=P, ldr=64, out16=P, ldo16=32)})
    # two rules broken: the earlier one answers
    r.update({"x=null, B<0": dict(x=None, B=-1), "B=0, x=null": dict(B=0, x=None), "B<0, K % 8": dict(B=-1, K=60), "K % 8, x misaligned": dict(K=60, x=P + 4),
              "W misaligned, unknown epilogue": dict(W=P + 4, epilogue=7), "N=0, K % 8": dict(N=0, K=60), "ldw % 8, N % 16": dict(ldw=68, N=24, ldo=24)})
    if norm:
        r.update({"ln_weight=null, x=null": dict(ln_weight=None, x=None), "RESIDUAL, B<0": dict(epilogue=1, B=-1)})
    if f16 and not norm:
        r["out16 with STORE, x=null"] = dict(out16=P, ldo16=64, x=None)
    return r


def _expert_rules():
    r = _nulls(["x", "W", "out", "expert"])
    r.update(_misaligned(["x", "W"]))
    r.update({"B=0": dict(B=0), "B<0": dict(B=-1), "B too large": dict(B=9), "N=0": dict(N=0), "K=0": dict(K=0), "K % 8": dict(K=60),
              "ldx short": dict(ldx=56), "ldw % 8": dict(ldw=68), "stride % 8": dict(w_expert_stride=64 * 64 + 4),
              "stride < N ldw": dict(w_expert_stride=2048), "E=0": dict(E=0), "E<0": dict(E=-1), "(E-1) stride overflows": dict(E=4, w_expert_stride=1 << 62),
              "RESIDUAL": dict(epilogue=1), "unknown epilogue": dict(epilogue=9), "ldo < N": dict(ldo=32),
              "SWIGLU N % 32": dict(epilogue=2, N=48), "SWIGLU ldo < N/2": dict(epilogue=2, ldo=16),
              "expert=null, B too large": dict(expert=None, B=9), "B too large, K % 8": dict(B=9, K=60), "K % 8, E=0": dict(K=60, E=0),
              "E=0, x misaligned": dict(E=0, x=P + 4), "x misaligned, RESIDUAL": dict(x=P + 4, epilogue=1), "RESIDUAL, ldo < N": dict(epilogue=1, ldo=32)})
    return r


def _append_rules(rows, rope):
    r = _nulls(["qkv", "cache_k", "cache_v", "lens"] + (["cos_tab", "sin_tab"] if rope else []) + (["cache_row"] if rows else []))
    r.update(_misaligned(["qkv", "cache_k", "cache_v"]))
    r.update({"B=0": dict(B=0), "B<0": dict(B=-1), "nq=0": dict(nq=0), "nkv=0": dict(nkv=0), "d % 8": dict(d=12), "Lmax=0": dict(Lmax=0),
              "qkv_stride % 8": dict(qkv_stride=1028),
              "qkv=null, B<0": dict(qkv=None, B=-1), "nq=0, qkv misaligned": dict(nq=0, qkv=P + 4), "B=0, qkv=null": dict(B=0, qkv=None)})
    if rope:
        r.update({"d % 16": dict(d=24), "qkv_stride too small": dict(qkv_stride=512), "qkv_stride too small, qkv misaligned": dict(qkv_stride=512, qkv=P + 4)})
    if rows:
        r.update({"cache_row=null, B=0": dict(cache_row=None, B=0)})
    return r


def _attn_rules(rows, rope):
    r = _nulls(["q", "cache_k", "cache_v", "lens", "out", "workspace"] + (["cos_tab", "sin_tab"] if rope else []) + (["cache_row"] if rows else []))
    r.update({"B=0": dict(B=0), "B<0": dict(B=-1), "B > 65535": dict(B=65536), "d=64": dict(d=64), "d=0": dict(d=0), "d > 65535": dict(d=65536),
              "Lmax=0": dict(Lmax=0), "Lmax > 32768": dict(Lmax=32769), "nq=0": dict(nq=0), "nq<0": dict(nq=-4), "nkv=0": dict(nkv=0),
              "nq > 65535": dict(nq=65536), "nkv > 65535": dict(nkv=65536, nq=65536), "nq % nkv": dict(nq=5),
              "16 heads per kv head": dict(nq=32, nkv=2, q_stride=8192, out_stride=4096),
              "q=null, d=64": dict(q=None, d=64), "d=64, B<0": dict(d=64, B=-1), "B<0, nq % nkv": dict(B=-1, nq=5),
              "nq % nkv, Lmax > 32768": dict(nq=5, Lmax=32769), "B=0, q=null": dict(B=0, q=None)})
    if rope:
        r.update({"q_stride too small": dict(q_stride=512), "cos_tab=null, B=0": dict(cos_tab=None, B=0), "nq=0, B=0": dict(nq=0, B=0),
                  "q_stride too small, B=0": dict(q_stride=512, B=0)})
    if rows:
        r.update({"cache_row=null, B=0": dict(cache_row=None, B=0)})
    return r


def _token_rules(sample):
    r = _nulls(["logits", "next"] + (["keys"] if sample else []))
    r.update({"B=0": dict(B=0), "B<0": dict(B=-1), "V=0": dict(V=0), "ld < V": dict(ld=1000), "ld % 8": dict(ld=1004),
              "history without step": dict(history=P, hist_stride=8), "logits misaligned": dict(logits=P + 4),
              "logits=null, V=0": dict(logits=None, V=0), "V=0, logits misaligned": dict(V=0, logits=P + 4), "B=0, logits=null": dict(B=0, logits=None)})
    if sample:
        r.update({"T=0": dict(temperature=0.0), "T<0": dict(temperature=-1.0), "T=inf": dict(temperature=INF), "T=nan": dict(temperature=NAN),
                  "top_p<0": dict(top_p=-0.1), "top_p>1": dict(top_p=1.5), "top_p=nan": dict(top_p=NAN), "top_k<0": dict(top_k=-1),
                  "T=0, B=0": dict(temperature=0.0, B=0), "top_p>1, top_k<0": dict(top_p=1.5, top_k=-1), "top_k<0, logits=null": dict(top_k=-1, logits=None)})
    return r


_WORKSPACE_CALLS = {"B=0": (0, 8, 2, 256), "nq=0": (2, 0, 2, 256), "nkv=0": (2, 8, 0, 256), "Lmax=0": (2, 8, 2, 0), "B<0": (-1, 8, 2, 256),
                    "B > 65535": (65536, 8, 2, 256), "nq > 65535": (2, 65536, 2, 256), "nkv > 65535": (2, 65536, 65536, 256),
                    "Lmax > 32768": (2, 8, 2, 32769), "gqa 4": (2, 8, 2, 256), "mha": (1, 4, 4, 8192), "gqa 3, Lmax % 64": (3, 6, 2, 100),
                    "gqa 8, Lmax 32768": (8, 32, 4, 32768)}
_COMBINE_RULES = dict(_nulls(["h", "h16", "y", "weights"]), **{"B=0": dict(B=0), "B<0": dict(B=-1), "B > 65535": dict(B=65536), "H=0": dict(H=0),
                                                               "B=0, h=null": dict(B=0, h=None), "h=null, H=0": dict(h=None, H=0)})

# entry point -> (argument names, valid call, rules)
ENTRY_POINTS = {
    "grit_gemv_bf16": (PROJ, _PROJ, _proj_rules(False, False, False)),
    "grit_gemv_f16": (PROJ_F16, _PROJ, _proj_rules(False, True, False)),
    "grit_rmsnorm_gemv_bf16": (NORM, _PROJ, _proj_rules(False, False, True)),
    "grit_rmsnorm_gemv_bf16_deferred": (NORM, _PROJ, _proj_rules(False, False, True)),
    "grit_rmsnorm_gemv_f16_deferred": (NORM, _PROJ, _proj_rules(False, True, True)),
    "grit_gemv_bf16_expert": (EXPERT, _EXPERT, _expert_rules()),
    "grit_gemv_f16_expert": (EXPERT, _EXPERT, _expert_rules()),
    "grit_decode_gemm_bf16": (PROJ, dict(_PROJ, B=9), _proj_rules(True, False, False)),
    "grit_decode_gemm_f16": (PROJ_F16, dict(_PROJ, B=9), _proj_rules(True, True, False)),
    "grit_rmsnorm_decode_gemm_bf16_deferred": (NORM, dict(_PROJ, B=9), _proj_rules(True, False, True)),
    "grit_rmsnorm_decode_gemm_f16_deferred": (NORM, dict(_PROJ, B=9), _proj_rules(True, True, True)),
    "grit_rope_kv_append": (ROPE_APPEND, _ATTN, _append_rules(False, True)),
    "grit_rope_kv_append_rows": (ROPE_APPEND_ROWS, _ATTN, _append_rules(True, True)),
    "grit_rope_kv_append_rows f16": (ROPE_APPEND_ROWS, dict(_ATTN, f16=1), _append_rules(True, True)),
    "grit_kv_append": (KV_APPEND, _ATTN, _append_rules(False, False)),
    "grit_attn_decode": (ATTN, _ATTN, _attn_rules(False, False)),
    "grit_attn_decode_rows": (ATTN_ROWS, _ATTN, _attn_rules(True, False)),
    "grit_attn_decode_rows f16": (ATTN_ROWS, dict(_ATTN, f16=1), _attn_rules(True, False)),
    "grit_attn_decode_rope": (ATTN_ROPE, _ATTN, _attn_rules(False, True)),
    "grit_attn_decode_rope_f16": (ATTN_ROPE, _ATTN, _attn_rules(False, True)),
    "grit_argmax_advance": (ARGMAX, _TOKEN, _token_rules(False)),
    "grit_argmax_advance_f32": (ARGMAX, _TOKEN, _token_rules(False)),
    "grit_sample_advance": (SAMPLE, _TOKEN, _token_rules(True)),
    "grit_sample_advance_f32": (SAMPLE, _TOKEN, _token_rules(True)),
    "grit_moe_decode_combine_f32": (COMBINE, _COMBINE, _COMBINE_RULES),
    "grit_attn_decode_workspace_floats": (WORKSPACE, {}, {k: dict(zip(WORKSPACE, v)) for k, v in _WORKSPACE_CALLS.items()}),
}


def table():
    """(entry of ENTRY_POINTS, rule, arguments in call order) of every call, in a fixed order"""
    for entry, (argnames, base, rules) in ENTRY_POINTS.items():
        for rule, change in rules.items():
            assert set(change) <= set(argnames), (entry, rule)
            a = dict(base, **change)
            yield entry, rule, [a[n] for n in argnames]


def _call(lib, entry, args):
    """(return value, error string) -- the size query has no error channel"""
    name = entry.split()[0]
    rc = int(getattr(lib, name)(*args))
    if name == "grit_attn_decode_workspace_floats" or rc == _lib.GRIT_OK:
        return rc, ""
    return rc, lib.grit_last_error_string().decode()


def _require_patterns(sources):
    """the message of every argument GRIT_REQUIRE in `sources` that a default build can reach, as a regular expression"""
    pats = []
    for src in sources:
        for m in re.finditer(r'GRIT_REQUIRE\(.*?,\s*GRIT_E_(?:BADARG|UNSUPPORTED),\s*"((?:[^"\\]|\\.)*)"', open(src).read(), flags=re.S):
            if any(u in m.group(1) for u in UNREACHABLE):
                continue
            pat = re.escape(m.group(1).replace("%%", "\0"))
            pat = re.sub(r"%(?:lld|d)", r"-?\\d+", pat).replace("%s", r"\w+").replace(re.escape("\0"), "%")
            if "^" + pat + "$" not in pats:
                pats.append("^" + pat + "$")
    return pats


def record(sources):
    lib = _lib.load()
    messages, calls = [], {}
    for entry, rule, args in table():
        rc, msg = _call(lib, entry, args)
        if entry != "grit_attn_decode_workspace_floats":
            assert rc in RECORDED_CODES, (entry, rule, rc, msg)      # no call of the table may reach a launch
            assert rc != _lib.GRIT_OK or "B=0" in rule, (entry, rule)
        if msg not in messages:
            messages.append(msg)
        calls.setdefault(entry, {})[rule] = [rc, messages.index(msg)]
    pats = _require_patterns(sources)
    missed = [p for p in pats if not any(re.match(p, m) for m in messages)]
    print(f"{sum(len(v) for v in calls.values())} calls, {len(messages)} distinct messages, {len(pats)} reachable GRIT_REQUIRE messages")
    print("GRIT_REQUIRE messages never hit:", missed)
    assert pats and not missed
    with open(GOLDEN, "w") as f:
        json.dump({"requires": pats, "messages": messages, "calls": calls}, f, indent=0, sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def golden():
    import torch
    if torch.cuda.is_available():
        pytest.skip("every call passes host pointers: run where no device can take a launch")
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_hits_every_require_of_the_recorded_entry_points(golden):
    assert len(golden["requires"]) == N_REQUIRES and set(golden["calls"]) == set(ENTRY_POINTS)
    for pat in golden["requires"]:
        assert any(re.match(pat, m) for m in golden["messages"]), pat
    for entry, recorded in golden["calls"].items():
        made = {rule for e, rule, _ in table() if e == entry}
        assert set(recorded) == made, sorted(set(recorded) ^ made)[:5]           # the recording and the table hold the same calls


@pytest.mark.parametrize("entry", list(ENTRY_POINTS))
def test_refusals_match_the_recording(golden, entry):
    lib = _lib.load()
    recorded = golden["calls"][entry]
    seen, wrong = 0, []
    for e, rule, args in table():
        if e != entry:
            continue
        want_rc, mi = recorded[rule]
        rc, msg = _call(lib, entry, args)
        seen += 1
        if (rc, msg) != (want_rc, golden["messages"][mi]):
            wrong.append((rule, rc, msg, want_rc, golden["messages"][mi]))
    assert seen == len(recorded) and seen > 0
    assert not wrong, (len(wrong), wrong[:8])


if __name__ == "__main__":
    assert sys.argv[1:3] == ["--record", "--source"] and len(sys.argv) > 3, __doc__
    record(sys.argv[3:])
