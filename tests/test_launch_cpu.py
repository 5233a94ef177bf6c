"""csrc/launch.h without a device: what a failed HIP call leaves for tw_last_hip_error() / tw_last_error_message().

A stand-alone program of two translation units, compiled for the host, records a failure in one and reads it in the
other (the library's eight sources share the state the same way); with no GPU, a launch through the library itself must
fail as TW_E_HIP and say which ABI function failed and why."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
TW_E_HIP = -2

RECORD = r"""
#include "launch.h"
int record(void) { return tw_fail(hipErrorInvalidValue, "ppo_age_scan", 7); }
"""

MAIN = r"""
#include <stdio.h>
#include "launch.h"
int record(void);
int main(void)
{
    if (g_last_hip_error != 0 || g_last_error_msg[0]) return 1;        /* clean before the first failure */
    const int rc = record();
    printf("%d\n%d\n%d\n%s\n%s\n", rc, g_last_hip_error, (int)hipErrorInvalidValue, g_last_error_msg,
           hipGetErrorString(hipErrorInvalidValue));
    return 0;
}
"""


def test_tw_fail_records_number_and_message():
    import twoarmy_amd
    with tempfile.TemporaryDirectory() as d:
        srcs = []
        for name, text in (("record.cpp", RECORD), ("main.cpp", MAIN)):
            srcs.append(os.path.join(d, name))
            with open(srcs[-1], "w") as f:
                f.write(text)
        exe = os.path.join(d, "launch_check")
        subprocess.check_call([HIPCC, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                               "-I", twoarmy_amd._lib.CSRC_DIR] + srcs + ["-o", exe])
        r = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    rc, number, invalid_value, message, text = r.stdout.splitlines()
    assert int(rc) == TW_E_HIP
    assert int(number) == int(invalid_value) != 0
    assert text and "ppo_age_scan" in message and text in message and "line 7" in message


def test_failed_launch_reports_itself_through_the_library():
    """No device: the launch of ppo_age_scan fails in HIP, and the library says so (before csrc/launch.h the PPO, view,
    render, obs, nav, visit and bonus families returned TW_E_HIP with hipError 0 and no text)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: failing launches are not provoked on a device")
    import twoarmy_amd
    lib = twoarmy_amd._lib.lib()
    cells = (C.c_int32 * 4)()
    p = C.cast(cells, C.c_void_p)
    assert lib.ppo_age_scan(p, p, p, 1, 1, p, None) == TW_E_HIP
    assert lib.tw_last_hip_error() != 0
    assert b"ppo_age_scan" in lib.tw_last_error_message()
    with pytest.raises(twoarmy_amd._lib.TwoarmyLibraryError, match=r"ppo_age_scan failed: rc=-2 hipError=[1-9]\d* ppo_age_scan"):
        twoarmy_amd._lib.check(TW_E_HIP, "ppo_age_scan")
