"""Random-argument fuzz of the C ABI WITHOUT a GPU (run it against the sanitizer build: tools/asan_host_shim.sh --fuzz): every grit_*
entry point gets null / misaligned / valid-looking host pointers and extreme sizes.  Nothing can be launched here (no device), so
the only things exercised are the host shim's validation and size arithmetic: a call must come back with an error code (or a
size), never crash, and the sanitizers must stay silent.     usage: fuzz_abi.py [seed] [calls per entry point] [log file]
With a log file every call leaves one line -- entry point, argument values (pointers by their offset into the scratch buffer), return
code, grit_last_error_string() -- so that two builds of the library can be compared refusal by refusal with `diff`."""
import ctypes as C, random, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gritlm_amd import _lib
lib = _lib.load()
random.seed(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
N = int(sys.argv[2]) if len(sys.argv) > 2 else 200
log = open(sys.argv[3], "w") if len(sys.argv) > 3 else None
lib.grit_last_error_string.restype = C.c_char_p
buf = (C.c_char * (1 << 16))()
addr = C.addressof(buf)
skip = {"grit_comm_init", "grit_comm_allgather_packed", "grit_comm_destroy", "grit_comm_unique_id", "grit_stream_create_cu_mask", "grit_stream_destroy"}
ints = [-1, 0, 1, 2, 7, 8, 32, 64, 128, 256, 4096, 14336, 2**31 - 1, -2**31]
longs = [-1, 0, 1, 64, 512, 4096, 131072, 2**40]
floats = [0.0, 1.0, -1.0, 1e-5, float("nan"), float("inf")]
total = 0; codes = {}
for name, (res, args) in _lib._SIGNATURES.items():
    if name in skip or not args: continue
    fn = getattr(lib, name)
    for _ in range(N):
        vals = []
        for a in args:
            if a is C.c_void_p: vals.append(random.choice([None, addr, addr + 16, addr + 1]))
            elif a is C.c_int: vals.append(random.choice(ints))
            elif a is C.c_int64: vals.append(random.choice(longs))
            elif a is C.c_float: vals.append(random.choice(floats))
            else: vals.append(None)
        r = fn(*vals)
        if log:
            shown = [("null" if v is None else f"buf+{v - addr}") if a is C.c_void_p else repr(v) for a, v in zip(args, vals)]
            log.write(f"{name}({', '.join(shown)}) -> {r} | {lib.grit_last_error_string().decode()}\n")
        total += 1
        codes[int(r) if r is not None else None] = codes.get(int(r) if r is not None else None, 0) + 1
# the expert-indexed GEMVs' stack description (ABI 6: E beside w_expert_stride) with every other argument valid: extreme E x stride pairs
# must be refused by the shim (E < 1, (E - 1) * stride beyond int64) before any launch
p16 = (addr + 15) & ~15
for name in ("grit_gemv_bf16_expert", "grit_gemv_f16_expert"):
    fn = getattr(lib, name)
    for _ in range(N):
        E = random.choice(ints + [3, 5, 16, 17])
        stride = random.choice(longs + [64 * 64, 2**62, 2**63 - 8])
        if not (E < 1 or (E > 1 and stride > (2**63 - 1) // (E - 1))):
            continue                  # a valid stack description would pass on to a launch: only the refused ones are called
        r = fn(p16, p16, p16, p16, stride, E, 1, 64, 64, 64, 64, 64, 0, None)
        total += 1
        codes[int(r)] = codes.get(int(r), 0) + 1
        assert r == _lib.GRIT_E_BADARG, (name, E, stride, r)
neg = {k: v for k, v in codes.items() if k is not None and k < 0}
print("calls", total, "negative return codes", dict(sorted(neg.items())), "zero", codes.get(0, 0), "positive", sum(v for k, v in codes.items() if k and k > 0))
