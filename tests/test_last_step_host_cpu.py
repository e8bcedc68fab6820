"""The host rules of a deferred last recursion step (lbfgspp_amd/csrc/last_step.hpp: when a product may end one step early,
which trial may run the step, and that every other reader of the direction runs it first), driven by a stand-alone program
without a device, built with AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_last_step_rules_under_sanitizers():
    bindir = os.path.join(ROOT, "tests", "cpp", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "test_last_step_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "cpp", "test_last_step_host.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout
