"""The device store's work areas on the CPU: every public *_work_size returns
what it has always returned, and every layout fits its size.

The sizes are pinned to literals recorded from a build of the commit before
the sizes came from the layouts (lzf_store_layout.h): a caller sizes its work
buffer with them, so they are part of the library's behaviour.  The layouts are
checked by csrc/carve_check.cpp, a stand-alone host program under the host
sanitizers; it is built and run here, never on a GPU and never inside Python."""
import os
import subprocess

import pytest

from tests.oracle_lib import ROOT

import gibson_amd

NS = (1, 2, 1023, 1024, 1025, 262145, 2**32 - 1)
VLENS = (1, 15, 16, 4096, 64 << 20)            # the last: LZF_GPU_MAX_VALUE
IN_BYTES = (0, 1, 2**20, 2**64 - 1)
SAT = 2**64 - 1

ONE_ARG = {
    "lzf_gpu_kv_frame_work_size": (113, 138, 25663, 25688, 25721, 6555761, 107374182455),
    "lzf_gpu_store_compact_work_size": (120, 136, 16472, 16488, 16528, 4200568, 68820140096),
    "lzf_gpu_store_select_work_size": (152, 152, 152, 152, 288, 34968, 570425360),
    "lzf_gpu_store_mget_work_size": (154, 212, 59430, 59488, 59562, 15208602, 249175212054),
    "lzf_gpu_store_replies_work_size": (146, 196, 51246, 51296, 51362, 13111442, 214815473694),
    "lzf_gpu_store_minc_work_size": (97, 106, 9295, 9304, 9321, 2361441, 38688260167),
    "lzf_gpu_store_keys_work_size": (96, 96, 96, 96, 112, 4192, 67108944),
}

# [n][vlen]
MSET = (
    (184, 200, 200, 4536, 71303352),
    (184, 200, 200, 4536, 71303352),
    (1192, 1208, 1208, 5544, 71304360),
    (1192, 1208, 1208, 5544, 71304360),
    (1216, 1232, 1232, 5568, 71304384),
    (264376, 264392, 264392, 268728, 71567544),
    (4328521888, 4328521904, 4328521904, 4328526240, 4399825056),
)

# [n][in_bytes]; the last column saturates
SET_STORE = (
    (132, 133, 1048708, SAT),
    (160, 161, 1048736, SAT),
    (28748, 28749, 1077324, SAT),
    (28776, 28777, 1077352, SAT),
    (28812, 28813, 1077388, SAT),
    (7342212, 7342213, 8390788, SAT),
    (120292638788, 120292638789, 120293687364, SAT),
)


def test_max_value_is_the_headers():
    src = open(os.path.join(ROOT, "include", "lzf_gpu.h")).read()
    assert "#define LZF_GPU_MAX_VALUE  (64u << 20)" in src


@pytest.mark.parametrize("name", sorted(ONE_ARG))
def test_work_size_of_one_argument(name):
    fn = getattr(gibson_amd.lib(), name)
    assert tuple(int(fn(n)) for n in NS) == ONE_ARG[name]


def test_mset_work_size():
    fn = gibson_amd.lib().lzf_gpu_store_mset_work_size
    assert tuple(tuple(int(fn(n, v)) for v in VLENS) for n in NS) == MSET


def test_set_store_work_size():
    fn = gibson_amd.lib().lzf_gpu_set_store_work_size
    assert tuple(tuple(int(fn(n, b)) for b in IN_BYTES) for n in NS) == SET_STORE


def test_every_layout_fits_its_size():
    csrc = os.path.join(ROOT, "gibson_amd", "csrc")
    subprocess.check_call(["make", "-s", "-C", csrc, "build/carve_check"])
    out = subprocess.run([os.path.join(csrc, "build", "carve_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "carve_check: ok" in out.stdout
