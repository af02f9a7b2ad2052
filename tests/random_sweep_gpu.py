#!/usr/bin/env python3
"""Random-shape parity sweep on the GPU beyond the 48 shapes of tests/test_gpu_parity.py: every shape's multiply
(+relinearise / modulus switch), relinearise and rotations against the C oracle (tests/full_size.py).
Test infrastructure (lives in tests/ because it uses the oracle).
Usage: python tests/random_sweep_gpu.py [seconds [first_idx [last_idx [ks_mode [big|f64|f64wide|devops|mbfv|- [emu]]]]]]   (big: N = 32768 / 65536 only;
f64: N = 4096 ... 16384 with every modulus below 2^50 -- the FP64-FMA kernels, round 6; f64wide: N = 8192 F64 launches of more
than one workgroup per CU -- the 512-thread key-switch instance; devops: the shapes of tests/devop_shapes.py through the device
encode, encrypt and key-generation cases against the Python restatements (tests/devop_cases.py), indices 0 ... 31 being tests;
mbfv: the same shapes through every multiparty share and aggregation against tests/mbfv_ref.py (mbfv_shape_cases.case_random_shape; a
single-modulus shape skips the relin rounds only), indices 0 ... 15 being tests;
emu: the same sweep on the host emulation of the kernel sources -- CPU CI evidence, no GPU needed)"""
import os, sys, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
from helpers import load_engine
import full_size
import devop_cases, devop_shapes, mbfv_shape_cases
engine = "emu" if len(sys.argv) > 6 and sys.argv[6] == "emu" else "hip"
fhe = load_engine(engine)
t0 = time.time(); done = 0; fails = []
budget = float(sys.argv[1]) if len(sys.argv) > 1 else 400
first = int(sys.argv[2]) if len(sys.argv) > 2 else 48
last = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
ks_mode = int(sys.argv[4]) if len(sys.argv) > 4 else 0      # fhe_ksk_set_mode of every key the sweep makes (0 = auto)
big = (sys.argv[5] if sys.argv[5] in ("big", "f64", "f64wide", "devops", "mbfv") else False) if len(sys.argv) > 5 else False   # "f64": shapes on the FP64-FMA kernels
with fhe.KeySwitchingKey.forced_mode(ks_mode):     # (thread-local, restored on exit)
    for idx in range(first, last):
        try:
            if big == "devops":
                devop_cases.check_random_shape(fhe, engine != "emu", idx)
            elif big == "mbfv":
                mbfv_shape_cases.case_random_shape(fhe, engine != "emu", idx)
            else:
                (full_size.check_random_shape_host if engine == "emu" else full_size.check_random_shape)(fhe, idx, big)
            done += 1
        except Exception as e:
            shape = devop_shapes.random_shape(idx) if big in ("devops", "mbfv") else full_size.random_shape(idx, big)
            fails.append((idx, shape, repr(e)[:200]))
            break
        if time.time() - t0 > budget: break
print(json.dumps({"engine": engine, "shapes_checked": done, "first_idx": first, "ks_mode": ks_mode, "big": big, "failures": fails, "seconds": round(time.time() - t0)}))
