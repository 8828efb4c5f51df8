"""Writes tests/golden/registration_<case>.npz: the problems of tests/registration_ref.CASES (fp32 inputs, the solver's
parameters) and what the reference's own teaser::RobustRegistrationSolver returns for them.  Build container only: compiles
tests/golden/make_registration_golden.cpp together with the reference's registration.cc against the TEASER++ headers and the
vendored Eigen of the reference's thirdparty tree (nothing of which is committed), runs it per case, parses its output.

    python tests/golden/make_registration_golden.py [--thirdparty DIR] [case ...]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from sage_slam_amd import build as sage_build  # noqa: E402
from tests import registration_ref as ref      # noqa: E402


def build_generator(thirdparty, out):
    teaser = os.path.join(thirdparty, "TEASER-plusplus", "teaser")
    # -DNDEBUG: a release build, as the reference ships (with its asserts the solver refuses N = 2: one pair)
    subprocess.check_call(["g++", "-O2", "-DNDEBUG", "-std=c++14", "-w", "-I" + os.path.join(teaser, "include"),
                           "-I" + os.path.join(thirdparty, "eigen"), os.path.join(HERE, "make_registration_golden.cpp"),
                           os.path.join(teaser, "src", "registration.cc"), "-o", out])


def run_case(gen, prob):
    p = prob["params"]
    lines = ["%d %.17g %.17g %d %.17g %.17g" % (prob["N"], p["noise_bound"], p["cbar2"], p["rotation_max_iterations"],
                                                p["rotation_cost_threshold"], p["rotation_gnc_factor"])]
    for s, d, b in zip(prob["src"], prob["dst"], prob["noise_bounds"]):
        lines.append(" ".join("%.9g" % float(v) for v in (*s, *d, b)))
    out = subprocess.run([gen], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    rec = {}
    for ln in out.splitlines():
        key, *vals = ln.split()
        rec[key] = vals
    return dict(valid=np.int32(rec["valid"][0]), scale=np.float64(rec["scale"][0]),
                R=np.array(rec["R"], np.float64).reshape(3, 3), t=np.array(rec["t"], np.float64),
                rotation_cost=np.float64(rec["rotation_cost"][0]), n_scale_inlier_pairs=np.int64(rec["scale_inliers"][0]),
                rotation_mask=np.array(rec["rotation_mask"], np.int32).astype(bool), inliers=np.array(rec["inliers"], np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--thirdparty", default=sage_build.REF_THIRDPARTY)
    ap.add_argument("cases", nargs="*")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        gen = os.path.join(tmp, "regen")
        build_generator(a.thirdparty, gen)
        for name in (a.cases or list(ref.CASES)):
            prob = ref.make_case(name)
            rec = dict(src=prob["src"], dst=prob["dst"], noise_bounds=prob["noise_bounds"],
                       params_names=np.array(sorted(prob["params"])), params_values=np.array([prob["params"][k] for k in sorted(prob["params"])], np.float64),
                       plant_scale=np.float64(prob["scale"]), plant_R=prob["R"], plant_t=prob["t"], outlier=prob["outlier"],
                       reference=np.bool_(ref.CASES[name]["reference"]))
            if ref.CASES[name]["reference"]:
                rec.update({"ref_" + k: v for k, v in run_case(gen, prob).items()})
            path = os.path.join(HERE, "registration_%s.npz" % name)
            np.savez_compressed(path, **rec)
            print(name, os.path.getsize(path), "bytes", "scale %.17g inliers %d" % (rec["ref_scale"], rec["ref_inliers"].size) if "ref_scale" in rec else "")


if __name__ == "__main__":
    main()
