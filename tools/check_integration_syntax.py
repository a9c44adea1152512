"""SYNTAX / TYPE CHECK ONLY of the reference-side adapter (integration/*.cc):  python tools/check_integration_syntax.py PATH/TO/mujoco_mpc

`g++ -std=c++20 -fsyntax-only` over the adapter sources against the reference's REAL mjpc/ headers (read where they lie in a
checkout of the reference, never copied) and declaration-only stand-ins for <mujoco/*.h> and <absl/*> (tests/stubs/): MuJoCo and
abseil are not needed, nothing is linked and nothing runs.  What it proves: the adapter overrides every pure virtual of
planners/planner.h with matching signatures, uses identifiers the reference really defines, and — third case — the reference's
own ilqs/planner.cc compiles UNCHANGED with SamplingPlanner swapped for HipSamplingPlanner (`sampling.trajectory[k]`,
`sampling.candidate_policy[k]`, `sampling.policy.plan...`).  It proves nothing about behaviour.  Outside the test suite because
it needs the reference's sources, which the repository does not carry.
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(ref, args):
    flags = ["g++", "-std=c++20", "-fsyntax-only", "-Werror=return-type", "-I" + os.path.join(ROOT, "tests", "stubs"), "-I" + ref,
             "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration")]
    return subprocess.run(flags + args, capture_output=True, text=True, timeout=300)


def adapter_compiles_against_reference_headers(ref, tmp):
    r = _check(ref, [os.path.join(ROOT, "integration", "hip_sampling_planner.cc")])
    return r.returncode == 0, r.stderr


def frozen_state_compiles_without_editing_the_reference(ref, tmp):
    # private ResidualFn members are read under -fno-access-control (integration/README.md): no friend lines needed
    r = _check(ref, ["-fno-access-control", os.path.join(ROOT, "integration", "frozen_state.cc")])
    return r.returncode == 0, r.stderr


def reference_ilqs_compiles_unchanged_on_top_of_the_adapter(ref, tmp):
    tu = os.path.join(tmp, "ilqs_on_hip.cc")
    with open(tu, "w") as f:
        f.write('#include "hip_sampling_planner.h"\n'
                '#include "mjpc/planners/sampling/planner.h"\n'          # the stock class keeps its name (include guard set)
                "#define SamplingPlanner HipSamplingPlanner\n"            # ... and iLQS's member `sampling` becomes the adapter
                '#include "mjpc/planners/ilqs/planner.h"\n'
                '#include "mjpc/planners/ilqs/planner.cc"\n')
    r = _check(ref, [tu])
    return r.returncode == 0, r.stderr


def the_check_really_checks(ref, tmp):
    # control: the identifiers round 2's adapter used do not exist in the reference and must be rejected
    tu = os.path.join(tmp, "wrong.cc")
    with open(tu, "w") as f:
        f.write('#include "hip_sampling_planner.h"\n#include "mjpc/planners/sampling/planner.h"\n'
                "double f() { return mjpc::MinNoiseStdSampling; }\n"
                "const mjpc::Trajectory& g(mjpc::HipSamplingPlanner& p) { return p.trajectory(3); }\n")
    r = _check(ref, [tu])
    return r.returncode != 0 and "MinNoiseStdSampling" in r.stderr and "trajectory" in r.stderr, r.stderr


CHECKS = [adapter_compiles_against_reference_headers, frozen_state_compiles_without_editing_the_reference,
          reference_ilqs_compiles_unchanged_on_top_of_the_adapter, the_check_really_checks]


def main(ref):
    if not os.path.isdir(os.path.join(ref, "mjpc")):
        raise SystemExit(f"{ref}: not a checkout of the reference (no mjpc/)")
    failed = 0
    with tempfile.TemporaryDirectory() as tmp:
        for check in CHECKS:
            ok, err = check(ref, tmp)
            print(("ok    " if ok else "FAIL  ") + check.__name__, flush=True)
            if not ok:
                failed += 1
                print(err[-4000:])
    raise SystemExit(1 if failed else 0)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(os.path.abspath(sys.argv[1]))
