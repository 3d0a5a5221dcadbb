"""CPU: the refusals of the six grit_attn_*_bwd entry points are ABI.  tests/golden/attn_bwd_abi_refusals.json holds, for a deterministic
table of calls with exactly one rule broken (and a few with two, which pin the ORDER of the rules), the return code and the error string
of the library the table was recorded from; the library under test must give the same code and a message that starts with the name of
the entry point that was called and, behind the first ": ", carries the recorded text.

Only refused calls (GRIT_E_BADARG, GRIT_E_UNSUPPORTED) are in the table: a call that passes validation launches.  Every call here passes
HOST pointers, so the module skips itself where a device is present: there a validation that lets one through would launch a kernel on
them; without a device such a call ends in GRIT_E_LAUNCH and fails the comparison.

Recording (from the revision whose behaviour is to be pinned; --source names that revision's csrc/attention_bwd.hip, whose GRIT_REQUIRE
messages -- all that a public entry can reach -- must be hit by the table):
    GRIT_HIP_LIB=<that revision's libgritlm_hip.so> python tests/test_attn_abi_cpu.py --record --source <its attention_bwd.hip>"""
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_bwd_abi_refusals.json")
REFUSALS = (_lib.GRIT_E_BADARG, _lib.GRIT_E_UNSUPPORTED)
# no public entry reaches this rule: the bidirectional and causal entries pass window = 0, the window entries refuse window < 1 themselves
UNREACHABLE = ("window=%d (causal attention only)",)

_buf = (ctypes.c_char * 4096)()
P = (ctypes.addressof(_buf) + 15) & ~15          # a 16-byte-aligned host address stands in for every pointer

PADDED = ["qkv", "key_bits", "out", "dout", "lse", "delta", "dqkv", "B", "S", "nq", "nkv", "d", "qkv_stride", "out_stride", "scale", "stream"]
VARLEN = ["qkv", "cu_seqlens", "out", "dout", "lse", "delta", "dqkv", "B", "S", "T", "nq", "nkv", "d", "qkv_stride", "out_stride", "scale", "stream"]
POINTERS = ["qkv", "mask", "out", "dout", "lse", "delta", "dqkv"]          # "mask": key_bits or cu_seqlens; "S": S or max_len
# a valid call: 2 sequences of 64 rows, 4 heads on 2 kv heads, rows longer than the heads need (so that nq = 5 breaks one rule only)
BASE = dict(qkv=P, mask=P, out=P, dout=P, lse=P, delta=P, dqkv=P, B=2, S=64, T=128, nq=4, nkv=2, d=128, qkv_stride=2048, out_stride=1024,
            scale=0.088, window=16, stream=None)


def _rules(varlen, window):
    r = {}
    for n in POINTERS:
        r[f"{n}=null"] = {n: None}
    for n in ("qkv", "out", "dout", "dqkv"):
        r[f"{n} misaligned"] = {n: P + 2}
    r.update({"B=0": dict(B=0), "B<0": dict(B=-1), "S=0": dict(S=0), "S<0": dict(S=-64), "nq=0": dict(nq=0), "nq<0": dict(nq=-4),
              "nkv=0": dict(nkv=0), "nkv<0": dict(nkv=-2), "S > 2^30": dict(S=(1 << 30) + 1), "nq > 65535": dict(nq=65536),
              "nkv > 65535": dict(nkv=65536, nq=65536),
              "d=64": dict(d=64), "d=256": dict(d=256), "d=0": dict(d=0), "nq % nkv": dict(nq=5),
              "qkv_stride % 8": dict(qkv_stride=2052), "qkv_stride short": dict(qkv_stride=1016), "out_stride % 8": dict(out_stride=1028),
              "out_stride short": dict(out_stride=504),
              "grid too large": dict(B=1 << 28), "grid too large by the blocks": dict(B=1 << 14, S=1 << 21, qkv_stride=1024, out_stride=512),
              "qkv rows span 2 GiB": dict(S=1 << 20), "out rows span 2 GiB": dict(S=1 << 19, qkv_stride=1024, out_stride=2048)})
    if varlen:
        r.update({"T=0": dict(T=0), "T<0": dict(T=-128)})
    if window:
        r.update({"window=0": dict(window=0), "window<0": dict(window=-1)})
    # two rules broken: the earlier one answers
    r.update({"qkv=null, B=0": dict(qkv=None, B=0), "dqkv=null, d=64": dict(dqkv=None, d=64), "S=0, d=64": dict(S=0, d=64),
              "d=64, nq % nkv": dict(d=64, nq=5), "nq % nkv, qkv_stride short": dict(nq=5, qkv_stride=1016),
              "out_stride % 8, out misaligned": dict(out_stride=1028, out=P + 2), "dout misaligned, grid too large": dict(dout=P + 2, B=1 << 28),
              "grid too large, rows span 2 GiB": dict(B=1 << 14, S=1 << 21), "lse=null, rows span 2 GiB": dict(lse=None, S=1 << 20)})
    if window:
        r.update({"window=0, qkv=null": dict(window=0, qkv=None), "window<0, d=64": dict(window=-1, d=64)})
    return r


# entry point -> (packed layout, takes a window)
ENTRY_POINTS = {
    "grit_attn_bidir_bwd": (False, False),
    "grit_attn_causal_bwd": (False, False),
    "grit_attn_causal_window_bwd": (False, True),
    "grit_attn_bidir_varlen_bwd": (True, False),
    "grit_attn_causal_varlen_bwd": (True, False),
    "grit_attn_causal_window_varlen_bwd": (True, True),
}


def table():
    """(entry point, rule, arguments by name) of every call, in a fixed order"""
    for name, (varlen, window) in ENTRY_POINTS.items():
        for rule, change in _rules(varlen, window).items():
            assert set(change) <= set(BASE), (name, rule)
            yield name, rule, dict(BASE, **change)


def _call(lib, name, a):
    varlen, window = ENTRY_POINTS[name]
    args = [a["qkv"], a["mask"], a["out"], a["dout"], a["lse"], a["delta"], a["dqkv"], a["B"], a["S"]] + ([a["T"]] if varlen else [])
    args += [a["nq"], a["nkv"], a["d"], a["qkv_stride"], a["out_stride"], a["scale"]] + ([a["window"]] if window else []) + [a["stream"]]
    rc = getattr(lib, name)(*args)
    return int(rc), (lib.grit_last_error_string().decode() if rc != _lib.GRIT_OK else "")


def _tail(msg):
    """the text behind the first ": " (the entry point's name stands in front of it)"""
    return msg.split(": ", 1)[1]


def _require_patterns(source):
    """the message of every GRIT_REQUIRE of the grit_attn_*_bwd entry points in `source` that a public entry can reach, as a regular
    expression"""
    pats = []
    for m in re.finditer(r'GRIT_REQUIRE\(.*?,\s*GRIT_E_(?:BADARG|UNSUPPORTED),\s*"(grit_attn_(?:[^"\\]|\\.)*)"', open(source).read(), flags=re.S):
        if any(u in m.group(1) for u in UNREACHABLE):
            continue
        pat = re.escape(m.group(1).replace("%%", "\0"))
        pat = re.sub(r"%(?:lld|d)", r"-?\\d+", pat).replace(re.escape("\0"), "%")
        pats.append("^" + pat + "$")
    return pats


def record(source):
    lib = _lib.load()
    messages, calls = [], {}
    for name, rule, args in table():
        rc, msg = _call(lib, name, args)
        assert rc in REFUSALS, (name, rule, rc, msg)          # every call of the table breaks a rule: none may reach a launch
        if msg not in messages:
            messages.append(msg)
        calls.setdefault(name, {})[rule] = [rc, messages.index(msg)]
    pats = _require_patterns(source)
    missed = [p for p in pats if not any(re.match(p, m) for m in messages)]
    print(f"{sum(len(v) for v in calls.values())} refusals, {len(messages)} distinct messages, {len(pats)} reachable GRIT_REQUIRE messages in {source}")
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
    assert len(golden["requires"]) == 18 and set(golden["calls"]) == set(ENTRY_POINTS)
    for pat in golden["requires"]:
        assert any(re.match(pat, m) for m in golden["messages"]), pat
    for name, recorded in golden["calls"].items():
        made = {rule for entry, rule, _ in table() if entry == name}
        assert set(recorded) == made, sorted(set(recorded) ^ made)[:5]           # the recording and the table hold the same calls


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_refusals_match_the_recording(golden, name):
    lib = _lib.load()
    recorded = golden["calls"][name]
    seen, wrong = 0, []
    for entry, rule, args in table():
        if entry != name:
            continue
        want_rc, mi = recorded[rule]
        want_msg = golden["messages"][mi]
        rc, msg = _call(lib, name, args)
        seen += 1
        if rc != want_rc:
            wrong.append((rule, "code", rc, want_rc, msg))
        elif not (msg.startswith(name + ": ") and _tail(msg) == _tail(want_msg)):
            wrong.append((rule, "message", msg, want_msg))
    assert seen == len(recorded) and seen > 0
    assert not wrong, (len(wrong), wrong[:8])


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"] and sys.argv[2:3] == ["--source"] and len(sys.argv) == 4, __doc__
    record(sys.argv[3])
