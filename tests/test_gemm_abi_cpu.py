"""CPU: the refusals of the eight grit_gemm_* entry points are ABI.  tests/golden/gemm_abi_refusals.json holds, for a deterministic table
of calls with exactly one rule broken (and a few with two, which pin the ORDER of the tests), the return code and the error string of the
library the table was recorded from; the library under test must give the same code, and a message that starts with the name of the
entry point that was called and keeps the substrings the Python layer and the other tests match.

Only calls the recorded library refused (GRIT_E_BADARG, GRIT_E_UNSUPPORTED) or answered with GRIT_OK for M == 0 are in the file.  Every
call here passes HOST pointers, so the module skips itself where a device is present: there a validation that lets one through would
launch a kernel on them; without a device such a call ends in GRIT_E_LAUNCH and fails the comparison.

Recording (from the revision whose behaviour is to be pinned; --source names that revision's csrc/gemm_bf16.hip, whose GRIT_REQUIRE
messages must all be hit by the table):
    GRIT_HIP_LIB=<that revision's libgritlm_hip.so> python tests/test_gemm_abi_cpu.py --record --source <its gemm_bf16.hip>"""
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_abi_refusals.json")
EPILOGUES = list(range(-1, 10))
RECORDED_CODES = (_lib.GRIT_OK, _lib.GRIT_E_BADARG, _lib.GRIT_E_UNSUPPORTED)
# what tests/test_abi.py and gritlm_amd/ match in the messages: a recorded message that has one of these keeps it
SUBSTRINGS = ("null pointer", "multiple of 64", "bad sizes", "bad leading dimensions", "16-byte aligned", "too many tiles", "residual",
              "not available", "unknown epilogue", "SWIGLU_STACKED_SAVE", "SWIGLU_BWD", "128")

_buf = (ctypes.c_char * 4096)()
P = (ctypes.addressof(_buf) + 15) & ~15          # a 16-byte-aligned host address stands in for every pointer
BIG = 1 << 40                                    # rows: 2^32 tiles of 256

DENSE = ["A", "W", "C", "M", "N", "K", "lda", "ldw", "ldc", "epilogue", "residual", "ldr", "stream"]
GROUPED = ["A", "a_rows", "W", "C", "group_counts", "num_groups", "M", "N", "K", "lda", "ldw", "w_group_stride", "ldc", "epilogue", "stream"]
GROUPED_EPI = ["A", "a_rows", "W", "C", "residual", "group_counts", "num_groups", "M", "N", "K", "lda", "ldw", "w_group_stride", "ldc", "ldr",
               "epilogue", "stream"]
ROPE = ["A", "W", "C", "M", "N", "K", "lda", "ldw", "ldc", "cos_tab", "sin_tab", "positions", "S", "table_rows", "rope_cols", "stream"]
PAIR = ["A1", "W1", "C1", "R1", "M1", "N1", "lda1", "ldw1", "ldc1", "ldr1", "A2", "W2", "C2", "R2", "M2", "N2", "lda2", "ldw2", "ldc2", "ldr2",
        "K", "epilogue", "stream"]

# base calls: every rule of every epilogue the entry point offers holds (M = 4, N = 256, K = 64; ldc = ldr = 2 N serves SWIGLU_BWD too)
_DENSE_BASE = dict(A=P, W=P, C=P, M=4, N=256, K=64, lda=64, ldw=64, ldc=512, residual=P, ldr=512, stream=None)
_GROUPED_BASE = dict(A=P, a_rows=None, W=P, C=P, group_counts=P, num_groups=2, M=4, N=256, K=64, lda=64, ldw=64, w_group_stride=256 * 64, ldc=512,
                     stream=None)
_ROPE_BASE = dict(A=P, W=P, C=P, M=4, N=256, K=64, lda=64, ldw=64, ldc=256, cos_tab=P, sin_tab=P, positions=None, S=8, table_rows=8,
                  rope_cols=128, stream=None)
_PAIR_BASE = dict(A1=P, W1=P, C1=P, R1=P, M1=4, N1=256, lda1=64, ldw1=64, ldc1=256, ldr1=256, A2=P, W2=P, C2=P, R2=P, M2=4, N2=256, lda2=64,
                  ldw2=64, ldc2=256, ldr2=256, K=64, stream=None)


def _pointer_rules(names):
    out = {}
    for n in names:
        out[f"{n}=null"] = {n: None}
        out[f"{n} misaligned"] = {n: P + 2}
    return out


def _ld_rules(names, short=56, odd=68):
    """a leading dimension below K (a multiple of 8) and one that is long enough but no multiple of 8"""
    out = {}
    for n in names:
        out[f"{n} short"] = {n: short}
        out[f"{n} % 8"] = {n: odd}
    return out


def _dense_rules(with_groups, with_residual):
    r = {"base": {}}
    r.update(_pointer_rules(["A", "W", "C"] + (["residual"] if with_residual else [])))
    if with_residual:
        r["residual misaligned by 4"] = {"residual": P + 4}
    r.update({"M=0, null pointers": dict(M=0, A=None, W=None, C=None), "M=0": dict(M=0), "M<0": dict(M=-1),
              "N=0": dict(N=0), "N<0": dict(N=-16), "N % 16": dict(N=248), "N % 64": dict(N=272),
              "K=0": dict(K=0), "K<0": dict(K=-64), "K % 64": dict(K=48, lda=48, ldw=48),
              "too many tiles": dict(M=BIG)})
    r.update(_ld_rules(["lda", "ldw"]))
    r.update({"ldc % 8": dict(ldc=516), "ldc < N/2": dict(ldc=120), "ldc < N": dict(ldc=248), "ldc < 2N": dict(ldc=504)})
    if with_residual:
        r.update({"ldr % 8": dict(ldr=516), "ldr % 4": dict(ldr=514), "ldr < N": dict(ldr=248), "ldr < 2N": dict(ldr=504)})
    if with_groups:
        r.update({"group_counts=null": dict(group_counts=None), "a_rows set": dict(a_rows=P), "num_groups=0": dict(num_groups=0),
                  "num_groups<0": dict(num_groups=-1), "num_groups=1025": dict(num_groups=1025),
                  "w_group_stride % 8": dict(w_group_stride=256 * 64 + 4),
                  "too many tiles with the groups": dict(M=((1 << 31) - 1024) * 256, num_groups=1024)})
    # two rules broken: the earlier test answers
    r.update({"A=null, M<0": dict(A=None, M=-1), "A=null, K % 64": dict(A=None, K=48), "M<0, K % 64": dict(M=-1, K=48),
              "K % 64, N % 16": dict(K=48, lda=48, ldw=48, N=248), "K % 64, lda short": dict(K=48, lda=40, ldw=48),
              "N % 16, ldw % 8": dict(N=248, ldw=68), "lda short, A misaligned": dict(lda=56, A=P + 2),
              "C misaligned, too many tiles": dict(C=P + 2, M=BIG), "too many tiles, ldc < N/2": dict(M=BIG, ldc=120),
              "N % 64, ldc < N/2": dict(N=272, ldc=120)})
    if with_residual:
        r["ldc < N/2, residual=null"] = dict(ldc=120, residual=None)
    if with_groups:
        r["num_groups=0, K % 64"] = dict(num_groups=0, K=48)
    return r


def _rope_rules():
    r = {"base": {}}
    r.update(_pointer_rules(["A", "W", "C", "cos_tab", "sin_tab"]))
    r.update({"M=0, null pointers": dict(M=0, A=None, W=None, C=None, cos_tab=None, sin_tab=None), "M<0": dict(M=-1),
              "N=0": dict(N=0), "N<0": dict(N=-256), "N % 128": dict(N=192, ldc=192), "K=0": dict(K=0), "K<0": dict(K=-64),
              "K % 64": dict(K=48, lda=48, ldw=48), "rope_cols % 128": dict(rope_cols=64), "rope_cols<0": dict(rope_cols=-128),
              "rope_cols > N": dict(rope_cols=384), "too many tiles": dict(M=BIG),
              "ldc < N": dict(ldc=248), "ldc % 8": dict(ldc=260),
              "neither positions nor S": dict(S=0), "S<0": dict(S=-1), "S > table rows": dict(S=16), "positions, no table rows": dict(positions=P, table_rows=0),
              "positions set": dict(positions=P, S=0)})
    r.update(_ld_rules(["lda", "ldw"]))
    r.update({"A=null, M<0": dict(A=None, M=-1), "K % 64, N % 128": dict(K=48, lda=48, ldw=48, N=192, ldc=192),
              "N % 128, lda short": dict(N=192, ldc=192, lda=56), "ldw % 8, W misaligned": dict(ldw=68, W=P + 2),
              "sin_tab misaligned, no S": dict(sin_tab=P + 2, S=0), "no S, too many tiles": dict(S=0, M=BIG)})
    return r


def _pair_rules():
    r = {"base": {}}
    r.update(_pointer_rules(["A1", "W1", "C1", "R1", "A2", "W2", "C2", "R2"]))
    r.update({"M1=0, null pointers": dict(M1=0, A1=None, W1=None, C1=None, R1=None), "M1=0": dict(M1=0), "M2=0": dict(M2=0), "M1<0": dict(M1=-1),
              "N1=0": dict(N1=0), "N2=0": dict(N2=0), "N2<0": dict(N2=-16), "N1 % 16": dict(N1=248, ldc1=248, ldr1=248), "N2 % 16": dict(N2=248, ldc2=248, ldr2=248),
              "K=0": dict(K=0), "K<0": dict(K=-64), "K % 64": dict(K=48, lda1=48, ldw1=48, lda2=48, ldw2=48),
              "too many tiles": dict(M1=BIG), "too many tiles in the sum": dict(M1=1 << 38, M2=1 << 38)})
    r.update(_ld_rules(["lda1", "ldw1", "lda2", "ldw2"]))
    r.update({"ldc1 < N1": dict(ldc1=248), "ldc2 < N2": dict(ldc2=248), "ldc1 % 8": dict(ldc1=260), "ldc2 % 8": dict(ldc2=260),
              "ldr1 < N1": dict(ldr1=248), "ldr2 < N2": dict(ldr2=248), "ldr1 % 8": dict(ldr1=260), "ldr2 % 8": dict(ldr2=260)})
    r.update({"A2=null, M1=0": dict(A2=None, M1=0), "M2=0, K % 64": dict(M2=0, K=48), "K % 64, ldw2 short": dict(K=48, ldw2=40),
              "N2 % 16, ldc2 % 8": dict(N2=248, ldc2=252), "ldc1 < N1, C1 misaligned": dict(ldc1=248, C1=P + 2),
              "W2 misaligned, too many tiles": dict(W2=P + 2, M1=BIG), "too many tiles, R1=null": dict(M1=BIG, R1=None)})
    return r


# entry point -> (argument names, base call, rules); the rope entry points take no epilogue argument
ENTRY_POINTS = {
    "grit_gemm_bf16_nt": (DENSE, _DENSE_BASE, _dense_rules(False, True)),
    "grit_gemm_f16_nt": (DENSE, _DENSE_BASE, _dense_rules(False, True)),
    "grit_gemm_bf16_nt_grouped": (GROUPED, _GROUPED_BASE, _dense_rules(True, False)),
    "grit_gemm_f16_nt_grouped": (GROUPED, _GROUPED_BASE, _dense_rules(True, False)),
    "grit_gemm_bf16_nt_grouped_epi": (GROUPED_EPI, dict(_GROUPED_BASE, residual=P, ldr=512), _dense_rules(True, True)),
    "grit_gemm_bf16_nt_rope": (ROPE, _ROPE_BASE, _rope_rules()),
    "grit_gemm_f16_nt_rope": (ROPE, _ROPE_BASE, _rope_rules()),
    "grit_gemm_bf16_nt_pair": (PAIR, _PAIR_BASE, _pair_rules()),
}


def table():
    """(entry point, rule, epilogue or None, arguments by name) of every call, in a fixed order"""
    for name, (argnames, base, rules) in ENTRY_POINTS.items():
        for rule, change in rules.items():
            assert set(change) <= set(base), (name, rule)
            for epi in (EPILOGUES if "epilogue" in argnames else [None]):
                yield name, rule, epi, dict(base, epilogue=epi, **change)


def _call(lib, name, args):
    rc = getattr(lib, name)(*(args[a] for a in ENTRY_POINTS[name][0]))
    return int(rc), (lib.grit_last_error_string().decode() if rc != _lib.GRIT_OK else "")


def _key(rule, epi):
    return rule if epi is None else f"{rule} | epilogue {epi}"


def _require_patterns(source):
    """the message of every GRIT_REQUIRE of the grit_gemm_* entry points in `source`, as a regular expression"""
    pats = []
    for m in re.finditer(r'GRIT_REQUIRE\(.*?,\s*GRIT_E_(?:BADARG|UNSUPPORTED),\s*"(grit_gemm_(?:[^"\\]|\\.)*)"', open(source).read(), flags=re.S):
        pat = re.escape(m.group(1).replace("%%", "\0"))
        pat = re.sub(r"%(?:lld|d)", r"-?\\d+", pat).replace(re.escape("\0"), "%")
        pats.append("^" + pat + "$")
    return pats


def record(source):
    lib = _lib.load()
    messages, calls = [], {}
    for name, rule, epi, args in table():
        rc, msg = _call(lib, name, args)
        if rc not in RECORDED_CODES or (rc == _lib.GRIT_OK and args.get("M", args.get("M1")) != 0):
            continue                          # a call this library would launch is not part of the table
        if msg not in messages:
            messages.append(msg)
        calls.setdefault(name, {})[_key(rule, epi)] = [rc, messages.index(msg)]
    pats = _require_patterns(source)
    missed = [p for p in pats if not any(re.match(p, m) for m in messages)]
    print(f"{sum(len(v) for v in calls.values())} refusals of {sum(1 for _ in table())} calls, {len(messages)} distinct messages, "
          f"{len(pats)} GRIT_REQUIRE messages in {source}")
    print("GRIT_REQUIRE messages never hit:", missed)
    assert not missed
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
    assert len(golden["requires"]) == 83 and set(golden["calls"]) == set(ENTRY_POINTS)
    for pat in golden["requires"]:
        assert any(re.match(pat, m) for m in golden["messages"]), pat
    keys = {name: set() for name in ENTRY_POINTS}
    for name, rule, epi, _ in table():
        keys[name].add(_key(rule, epi))
    for name, recorded in golden["calls"].items():
        assert set(recorded) <= keys[name], sorted(set(recorded) - keys[name])[:5]        # nothing recorded that the table no longer makes


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_refusals_match_the_recording(golden, name):
    lib = _lib.load()
    recorded = golden["calls"][name]
    seen, wrong = 0, []
    for entry, rule, epi, args in table():
        if entry != name or _key(rule, epi) not in recorded:
            continue
        want_rc, mi = recorded[_key(rule, epi)]
        want_msg = golden["messages"][mi]
        rc, msg = _call(lib, name, args)
        seen += 1
        if rc != want_rc:
            wrong.append((rule, epi, "code", rc, want_rc, msg))
        elif rc != _lib.GRIT_OK and not (msg.startswith(name + ":") and all(s in msg for s in SUBSTRINGS if s in want_msg)):
            wrong.append((rule, epi, "message", msg, want_msg))
    assert seen == len(recorded) and seen > 0
    assert not wrong, (len(wrong), wrong[:8])


if __name__ == "__main__":
    assert sys.argv[1:2] == ["--record"] and sys.argv[2:3] == ["--source"] and len(sys.argv) == 4, __doc__
    record(sys.argv[3])
