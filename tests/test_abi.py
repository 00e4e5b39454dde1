"""-m "not gpu": the C-ABI library loads, exports every declared symbol and fails loudly without a GPU."""
import ctypes as C
import os
import re

import pytest

from alego_amd import binding, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "alego_mi355x.h")).read()
    declared = set(re.findall(r"\b(alego_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"alego_default_params"}  # static inline in alego_params.h
    L = binding.lib()
    missing = [s for s in sorted(declared) if not hasattr(L, s)]
    assert not missing, f"libalego_mi355x.so lacks {missing}"
    assert set(binding.EXPORTS) == declared, (set(binding.EXPORTS) ^ declared)


def test_params_struct_matches_header():
    assert binding.lib().alego_params_sizeof() == C.sizeof(binding.AlegoParams)
    assert synth.lib().alego_synth_params_sizeof() == C.sizeof(binding.AlegoParams)


def test_no_cpu_fallback(params_a):
    """Without a gfx950 device alego_create must refuse (no oracle / CPU path behind the product API)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    assert binding.lib().alego_device_count() == 0
    with pytest.raises(binding.AlegoError):
        binding.Handle(params_a)


def test_product_does_not_link_the_oracle():
    """The shipped library and package never reference oracle/ (only tests, smoke and bench's cpu_baseline may)."""
    pkg = os.path.join(ROOT, "a-lego-loam_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".sh")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle_py" not in txt and "liboracle" not in txt and "oracle/" not in txt.replace("// oracle/", ""), f
    so = open(binding.lib_path(), "rb").read()
    assert b"liboracle" not in so
    # neither do the host-side sources around it: the development tools, the C++ example, the ROS adapters, the headers
    for sub in ("tools", "examples", "ros_adapter", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, sub)):
            for f in files:
                if f.endswith((".py", ".hip", ".h", ".cpp", ".sh")):
                    txt = open(os.path.join(dirpath, f), errors="ignore").read()
                    assert "oracle_py" not in txt and "liboracle" not in txt and "from oracle" not in txt, os.path.join(sub, f)


def test_device_memory_has_one_owner():
    """Device memory is taken and returned in one place: csrc/dev_mem.h (DevPool, DevBuf) on top of csrc/guard_alloc.cpp.  No other file under
    csrc/ names the runtime's allocator or the guard functions; guard_alloc.h, which declares the latter, names them and nothing else of these."""
    csrc = os.path.join(ROOT, "a-lego-loam_amd", "csrc")
    allowed = {"hipMalloc": {"guard_alloc.cpp"}, "hipFree": {"guard_alloc.cpp"},
               "guard_malloc": {"guard_alloc.cpp", "guard_alloc.h", "dev_mem.h"}, "guard_free": {"guard_alloc.cpp", "guard_alloc.h", "dev_mem.h"}}
    files = sorted(os.listdir(csrc))
    assert "dev_mem.h" in files and "guard_alloc.cpp" in files
    for f in files:
        txt = open(os.path.join(csrc, f), errors="ignore").read()
        for name, where in allowed.items():
            assert name not in txt or f in where, f"{f} names {name}"


FRONT_END_ARRAYS = ("scal", "feat", "feat_idx", "feat_cnt", "ring_off", "ring_boff", "lo_box", "lo_cpts", "lo_cell", "lo_geom", "lo_corr", "st_idx", "st_cnt",
                    "st_lfds", "row_cnt", "ipb_col", "ipb_off", "poses", "traj", "traj_n", "lo_state", "imu_ring", "imu_ptr", "ring_start", "ring_end", "ori",
                    "fe_sync")


def test_front_end_arrays_have_one_layout():
    """The layout of DevCtx's structured per-slot arrays is defined in one place: csrc/fe_store.h.  No other file under csrc/ indexes or offsets one of
    them (the member followed by `[` or `+`; a null test and the address taken for allocation remain), and none multiplies by SC_COUNT, LO_STATE_N or
    ALEGO_IMU_Q."""
    import re
    csrc = os.path.join(ROOT, "a-lego-loam_amd", "csrc")
    files = sorted(os.listdir(csrc))
    assert "fe_store.h" in files
    member = re.compile(r"(?:\.|->)\s*(" + "|".join(FRONT_END_ARRAYS) + r")\s*[\[+]")
    address = re.compile(r"&\s*[\w.>-]*(?:\.|->)(feat|feat_idx|lo_cpts)\[\w+\]\s*[,)]")   # &d.feat[k] handed to the allocator: the member arrays of pointers
    stride = re.compile(r"\*\s*(SC_COUNT|LO_STATE_N|ALEGO_IMU_Q)\b|\b(SC_COUNT|LO_STATE_N|ALEGO_IMU_Q)\s*\*")
    bad = []
    for f in files:
        if f == "fe_store.h":
            continue
        for no, line in enumerate(open(os.path.join(csrc, f), errors="ignore"), 1):
            code = address.sub("", line.split("//")[0])
            if member.search(code) or stride.search(code):
                bad.append(f"{f}:{no}: {line.strip()[:120]}")
    assert not bad, "\n".join(bad)


def test_icp_attempts_have_one_definition():
    """What an ICP attempt of alego_loop_search, the appearance search and relocalisation is made of is defined once: a frame's clouds in kf_store.h
    (KfClouds), the archive gather, the window, the rounds and the result in loop_ctx.h / kernels_loop.hip, the candidate word in reloc_math.h, the
    workgroup arg-min in wave.h, "get from a pool or set the error" in dev_mem.h.  The copies these replaced are named nowhere under csrc/, and no
    code outside reloc_math.h takes a candidate word apart or puts one together by hand."""
    csrc = os.path.join(ROOT, "a-lego-loam_amd", "csrc")
    text = {f: open(os.path.join(csrc, f), errors="ignore").read() for f in sorted(os.listdir(csrc))}
    assert {"kernels_reloc.hip", "kernels_loop.hip", "reloc_math.h", "kf_store.h", "loop_ctx.h", "wave.h", "dev_mem.h"} <= set(text)
    for f, txt in text.items():
        for gone in ("la_gather", "rl_alloc", "lc_alloc", "rl_block_min"):
            assert gone not in txt, f"{f} names {gone}"
    assert "LI_NCUR_" not in text["kernels_reloc.hip"], "the current scan's clouds are read through kf_clouds_cur"
    bad = []
    for f, txt in text.items():
        if f == "reloc_math.h":
            continue
        code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), txt, flags=re.S))
        for no, line in enumerate(code.split("\n"), 1):
            by8 = re.search(r"(>>|<<)\s*8\b", line)
            if ("0xffffffu" in line.lower() and by8) or (re.search(r"<<\s*32\b", line) and by8):   # id = (c >> 8) & 0xffffff; D << 32 | id << 8 | s
                bad.append(f"{f}:{no}: {line.strip()[:120]}")
    assert not bad, "\n".join(bad)
    kernels = re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)\s*\(", text["kernels_reloc.hip"])
    assert len(kernels) >= 10 and [k for k in kernels if k.endswith("_gather")] == ["rl_gather"], kernels
    for name, where in (("KfClouds", "kf_store.h"), ("lc_window", "reloc_math.h"), ("rl_cand_pack", "reloc_math.h"), ("block_min_u64", "wave.h"), ("DevGet", "dev_mem.h"),
                        ("loop_rounds", "loop_ctx.h"), ("loop_archive_gather", "loop_ctx.h"), ("loop_result_fill", "loop_ctx.h")):
        assert name in text[where], f"{where} defines {name}"


def test_cpp_example_fails_loudly_without_a_gpu():
    """examples/replay.cpp drives the C ABI from plain C++.  In a container without an MI355X it must stop at alego_create with
    ALEGO_ERR_NO_DEVICE — there is no CPU fallback for the product path (on the GPU box tests/test_gpu_parity.py runs it for real)."""
    import subprocess
    exe = os.path.join(ROOT, "examples", "replay")
    assert os.path.exists(exe), "__graft_entry__.build() compiles it"
    r = subprocess.run([exe, "2"], capture_output=True, text=True, timeout=120)
    if r.returncode == 0:
        pytest.skip("a GPU is present")
    assert r.returncode == 1 and "no CPU fallback" in r.stderr, (r.returncode, r.stderr)
