"""The pure host parts of the refine drivers under ASan / UBSan: tools/job_sanitize.cpp -- the packed layouts (box_area, box_slot, cloud_slot),
the plan of an asynchronous batch (plan_async), the overlap rule (release_pass_for), the byte rule of a timed pass (icp_span_bytes), the
mixed-batch layer (plan_meshes, Batch, camera_centers), the scene caches (the control words NNInfo, FpWords and ProjTail at their documented
positions, packed_layout, the source lists, the set choice pick_nn_set and the route choice nn_route of make_scene), beside the job, request and workspace checks it already held -- built with the command in its own first line as a stand-alone program and run.  Nothing is
loaded into this process and no device is needed."""
import os
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join("tools", "job_sanitize.cpp")


def build_command(out: str) -> list:
    """The compile command of the source's first line ('// build: g++ ... -o job_sanitize;  ./job_sanitize'), writing to `out`."""
    with open(os.path.join(ROOT, SOURCE)) as f:
        first = f.readline()
    assert first.startswith("// build: "), first
    cmd = shlex.split(first[len("// build: "):].split(";")[0])
    assert cmd[0] == "g++" and SOURCE in cmd and "-fsanitize=address,undefined" in cmd and cmd[-2] == "-o", cmd
    return cmd[:-1] + [out]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++ on this machine")
def test_job_sanitize_runs_clean(tmp_path):
    exe = str(tmp_path / "job_sanitize")
    built = subprocess.run(build_command(exe), cwd=ROOT, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], cwd=ROOT, capture_output=True, text=True)
    print(ran.stdout, ran.stderr)
    assert ran.returncode == 0, (ran.stdout[-2000:], ran.stderr[-2000:])
    assert "job_sanitize: ok" in ran.stdout.splitlines()
