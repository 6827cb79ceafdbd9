#!/usr/bin/env python
"""Host sanitizer run of mpn_prn_match_host on the limit cases of tests/test_prn_assign_parity_cpu.py (CPU only, no GPU needed).

Builds csrc/prn_assign.hip with AddressSanitizer and UndefinedBehaviorSanitizer on its HOST code only, links it with main.cpp into a
stand-alone program, runs that program on every case (65 boxes, 64 / 65 / 520 / 600 distinct ids, cand_n > cap, and the generated
scenes) and compares its out_kp / tie_flags with the production library's.  The sanitized code is never loaded into python.

    python tools/prn_match_sanitize/run.py            # prints one line per case, exits non-zero on any report or mismatch
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SAN = "-fsanitize=address,undefined"


def build(out_dir):
    hipcc = os.path.join(ROCM, "bin", "hipcc")
    clang = os.path.join(ROCM, "lib", "llvm", "bin", "clang++")
    csrc = os.path.join(ROOT, "multiposenet", "pytorch_amd", "csrc")
    obj, main_o, exe = (os.path.join(out_dir, n) for n in ("prn_assign.o", "main.o", "prn_match_sanitized"))
    common = ["-O1", "-g", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", csrc]
    # device code is compiled as always; only the host half carries the sanitizers
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Xarch_host", SAN] + common +
                          ["-c", os.path.join(csrc, "prn_assign.hip"), "-o", obj])
    subprocess.check_call([clang, "-std=c++17", SAN] + common + ["-c", os.path.join(HERE, "main.cpp"), "-o", main_o])
    subprocess.check_call([clang, SAN, obj, main_o, "-L", os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", exe])
    return exe


def dump(path, a, cn, ci, cs, amax, cap):
    nimg, nb = len(a["box_start"]) - 1, a["boxes"].shape[0]
    with open(path, "wb") as f:
        np.array([nimg, nb, len(a["peaks"]), cap, 56, 36], dtype=np.int32).tofile(f)
        for arr, dt in ((a["box_start"], np.int32), (a["boxes"], np.float64), (a["joint_off"], np.int32), (a["peaks"], np.float64), (cn, np.int32),
                        (ci, np.int32), (cs, np.float32), (amax, np.int32)):
            np.ascontiguousarray(arr, dtype=dt).tofile(f)


def main():
    import prn_assign_ref as R
    import test_prn_assign_parity_cpu as T
    cases = [(name, sc, cap) for name, (sc, cap, _, _) in T.limit_cases().items()]
    cases += [("normal scene", R.normal_scene(), 64), ("dense scene", R.dense_scene(), 64), ("dense scene, cap 2048", R.dense_scene(), 2048),
              ("crowded scene", R.crowded_scene(77, nimg=4), 64)]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        for name, sc, cap in cases:
            nb = sum(len(b) for b in sc.boxes)
            out = np.random.RandomState(5).uniform(0.01, 1.0, (nb, 56, 36, 17)).astype(np.float32)
            cn, ci, cs, _ = R.ref_candidates(out, R.scene_maps(sc)["occ"], 15, cap)
            amax = R.ref_argmax(out)
            a = sc.arrays()
            want_kp, want_fl = R.match_host(a, cn, ci, cs, cap, amax)
            dump(os.path.join(tmp, "case.bin"), a, cn, ci, cs, amax, cap)
            p = subprocess.run([exe, os.path.join(tmp, "case.bin"), os.path.join(tmp, "res.bin")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            ok = p.returncode == 0 and not p.stdout.strip()
            if ok:
                raw = open(os.path.join(tmp, "res.bin"), "rb").read()
                kp = np.frombuffer(raw[:nb * 51 * 8], dtype=np.float64).reshape(nb, 17, 3)
                fl = np.frombuffer(raw[nb * 51 * 8:], dtype=np.uint8).reshape(sc.nimg, 17)
                ok = np.array_equal(kp, want_kp) and np.array_equal(fl, want_fl)
            print("%-24s boxes %3d cap %4d flagged %2d  %s" % (name, nb, cap, int(want_fl.sum()), "clean, equal to the library" if ok else "FAILED"))
            if not ok:
                bad += 1
                sys.stdout.write(p.stdout.decode(errors="replace")[-4000:])
    print("%d cases, %d failed" % (len(cases), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
