"""CPU test of the drop-in boundary, HipHeadlessRenderer::render (csrc/host/headless.cpp): its stand-alone program."""
import importlib
import os
import subprocess

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "metal-pathtracer-arm64_amd")


def test_headless_check_program(tmp_path):
    """tools/headless_check.cpp: every refusal of render()'s plan comes back with exactly its message and before any device call - the two
    snapshot lists {8,4} and {4,16} at 16 spp too, which used to get as far as the scene upload - and, without a device, every frame kind
    alone, with feature buffers, with the denoiser and with its sample variance ends with the device check's message and a clean exit."""
    exe = str(tmp_path / "headless_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc", "host"),
                            os.path.join(ROOT, "tools", "headless_check.cpp"), "-L" + PKG, "-lptr_hip", "-Wl,-rpath," + PKG, "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run(["timeout", "-k", "2", "60", exe, os.path.join(ROOT, "tests", "golden", "smoke.scene")], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    lines = run.stdout.splitlines()
    assert lines[-1] == "0 finding(s) in all"
    assert sum(l.startswith("ok      refusal-") for l in lines) == 7
    if pt.device_count() == 0:
        assert sum(l.startswith("ok      no-device-") and "no CPU fallback" in l for l in lines) == 15
