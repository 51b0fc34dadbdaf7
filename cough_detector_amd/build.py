"""Build libcough_amd.so and its companions libcough_amd_loop.so, libcough_amd_data.so, libcough_amd_segments.so,
libcough_amd_score.so, libcough_amd_draws.so, libcough_amd_warp.so, libcough_amd_pitch.so and libcough_amd_soft.so (HIP,
gfx950 only) in-tree with hipcc.

Every translation unit is compiled to an object file of its own (in parallel, cached under ``build/`` by the newest
source / header time) and the objects are linked into the shared libraries: ``SOURCES`` into ``libcough_amd.so`` (the
C-ABI of ``include/cough_amd.h``), ``LOOP_SOURCES`` into ``libcough_amd_loop.so`` (``include/cough_amd_loop.h``),
``DATA_SOURCES`` into ``libcough_amd_data.so`` (``include/cough_amd_data.h``), ``SEGMENTS_SOURCES`` into
``libcough_amd_segments.so`` (``include/cough_amd_segments.h``), ``SCORE_SOURCES`` into ``libcough_amd_score.so``
(``include/cough_amd_score.h``), ``DRAWS_SOURCES`` into ``libcough_amd_draws.so`` (``include/cough_amd_draws.h``), ``WARP_SOURCES`` into
``libcough_amd_warp.so`` (``include/cough_amd_warp.h``), ``PITCH_SOURCES`` into ``libcough_amd_pitch.so``
(``include/cough_amd_pitch.h``), ``SOFT_SOURCES`` and the three training
translation units compiled a second time with ``SOFT_FLAGS`` into ``libcough_amd_soft.so`` (``include/cough_amd_soft.h``).  The libraries are build products and stay out of git.
Usage: ``python -m cough_detector_amd.build [--force]``.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "libcough_amd.so")
SOURCES = ("api.hip", "featurize.hip", "featurize_generic.hip", "spectrogram.hip", "resnet.hip", "cnn.hip", "stream.hip", "synth.hip",
           "augment.hip", "train.hip", "train_small.hip", "train_std.hip")
# the companion library of the epoch loop: include/cough_amd.h stays at ABI v5 with its 53 entry points, so what the
# loop adds is exported from a library of its own (same flags, a version script of its own)
LOOP_LIB = os.path.join(HERE, "libcough_amd_loop.so")
LOOP_SOURCES = ("loop.hip",)
# the companion library of the input pipeline (the device-resident dataset and batch loader), on the same terms
DATA_LIB = os.path.join(HERE, "libcough_amd_data.so")
DATA_SOURCES = ("data.hip",)
# the companion library of corpus curation (frame energies, segment picking), on the same terms
SEGMENTS_LIB = os.path.join(HERE, "libcough_amd_segments.so")
SEGMENTS_SOURCES = ("segments.hip",)
# the companion library of offline scoring (deque mean, threshold sweep, event list), on the same terms
SCORE_LIB = os.path.join(HERE, "libcough_amd_score.so")
SCORE_SOURCES = ("score.hip",)
# the companion library of the device-side draws (a batch's augmentation records and masks, augmentation from them), on
# the same terms; it compiles csrc/augment_kernel.h, the kernel augment.hip runs
DRAWS_LIB = os.path.join(HERE, "libcough_amd_draws.so")
DRAWS_SOURCES = ("draws.hip",)
# the companion library of speed perturbation (the tableless per-row sinc resampler and its draws), on the same terms
WARP_LIB = os.path.join(HERE, "libcough_amd_warp.so")
WARP_SOURCES = ("warp.hip",)
# the companion library of pitch shift (the per-row float64 phase vocoder and its draws), on the same terms
PITCH_LIB = os.path.join(HERE, "libcough_amd_pitch.so")
PITCH_SOURCES = ("pitch.hip",)
# the companion library of the soft-target training steps and the batch MixUp, on the same terms.  Its three steps are
# the training translation units of libcough_amd.so compiled a second time: SOFT_FLAGS only selects which extern "C"
# functions they emit (the *_forward_backward_soft entry points instead of the v5 ones), so the step code exists once
SOFT_LIB = os.path.join(HERE, "libcough_amd_soft.so")
SOFT_SOURCES = ("soft.hip",)
SOFT_SHARED_SOURCES = ("train.hip", "train_small.hip", "train_std.hip")
SOFT_FLAGS = ("-DCOUGH_SOFT_EXPORTS",)
# -fno-slp-vectorize: left alone, -O3 packs adjacent f32 adds / multiplies of the FFT butterflies into v_pk_*_f32, which issue
# slower than the two scalar operations they replace on gfx950 (same-box A/B: K1 -2.4 %, STFT stage -3.2 %, classifier unchanged;
# profiles/r04_flag_ab.txt)
# -fvisibility=hidden: the shared object exports the entry points include/cough_amd.h declares (its `#pragma GCC visibility
# push(default)`) and nothing else -- no C++-mangled internals, no std::vector instantiations
CFLAGS = ["-O3", "-std=c++20", "--offload-arch=gfx950", "-fPIC", "-Wall", "-Wno-unused-function", "-fno-slp-vectorize",
          "-fvisibility=hidden", "-fvisibility-inlines-hidden"]
FLAGS = CFLAGS + ["-shared"]          # one-shot command line (the diagnostic tools build variants with it)


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm with gfx950 support)")


def _headers_mtime() -> float:
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    deps += [os.path.join(HERE, "..", "include", h) for h in ("cough_amd.h", "cough_amd_loop.h", "cough_amd_data.h",
                                                                   "cough_amd_segments.h", "cough_amd_score.h",
                                                                   "cough_amd_draws.h", "cough_amd_soft.h",
                                                                   "cough_amd_warp.h", "cough_amd_pitch.h")]
    deps.append(os.path.abspath(__file__))   # the flags live here
    deps += [os.path.join(CSRC, m) for m in ("exports.map", "exports_loop.map", "exports_data.map", "exports_segments.map",
                                             "exports_score.map", "exports_draws.map", "exports_soft.map",
                                             "exports_warp.map", "exports_pitch.map")]
    return max(os.path.getmtime(d) for d in deps)


def is_stale() -> bool:
    libs = (LIB, LOOP_LIB, DATA_LIB, SEGMENTS_LIB, SCORE_LIB, DRAWS_LIB, SOFT_LIB, WARP_LIB, PITCH_LIB)
    if not all(os.path.exists(p) for p in libs):
        return True
    t = min(os.path.getmtime(p) for p in libs)
    return _headers_mtime() > t or any(os.path.getmtime(os.path.join(CSRC, s)) > t
                                       for s in SOURCES + LOOP_SOURCES + DATA_SOURCES + SEGMENTS_SOURCES + SCORE_SOURCES
                                       + DRAWS_SOURCES + SOFT_SOURCES + WARP_SOURCES + PITCH_SOURCES)


def build_library(force: bool = False, verbose: bool = True, extra_flags=(), out: str = LIB) -> str:
    """Compile (only what changed, unless ``force`` / ``extra_flags``) and link the libraries.  ``extra_flags`` (e.g.
    ``-DCOUGH_K1_STAMPS``) build a variant of libcough_amd.so alone at ``out`` with objects of its own."""
    if not force and not extra_flags and not is_stale():
        return LIB
    hipcc = _hipcc()
    objdir = OBJ if not extra_flags else OBJ + "_" + str(abs(hash(tuple(extra_flags))) % 10**8)
    os.makedirs(objdir, exist_ok=True)
    hdr = _headers_mtime()

    def compile_one(job) -> str:
        src, flags, suffix = job if isinstance(job, tuple) else (job, (), "")
        s, o = os.path.join(CSRC, src), os.path.join(objdir, src.replace(".hip", suffix + ".o"))
        if force or not os.path.exists(o) or os.path.getmtime(o) < max(hdr, os.path.getmtime(s)):
            cmd = [hipcc, *CFLAGS, *extra_flags, *flags, "-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
        return o

    def link(objs, version_script: str, target: str) -> None:
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC",
               "-Wl,--version-script=" + os.path.join(CSRC, version_script), "-o", target, *objs]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    variant = bool(extra_flags) or out != LIB
    sources = SOURCES if variant else (SOURCES + LOOP_SOURCES + DATA_SOURCES + SEGMENTS_SOURCES + SCORE_SOURCES
                                      + DRAWS_SOURCES + WARP_SOURCES + PITCH_SOURCES + SOFT_SOURCES
                                      + tuple((src, SOFT_FLAGS, "_soft") for src in SOFT_SHARED_SOURCES))
    with ThreadPoolExecutor(max_workers=min(len(sources), os.cpu_count() or 1)) as pool:
        objs = list(pool.map(compile_one, sources))
    link(objs[:len(SOURCES)], "exports.map", out)
    if not variant:
        link(objs[len(SOURCES):len(SOURCES) + len(LOOP_SOURCES)], "exports_loop.map", LOOP_LIB)
        data_end = len(SOURCES) + len(LOOP_SOURCES) + len(DATA_SOURCES)
        link(objs[len(SOURCES) + len(LOOP_SOURCES):data_end], "exports_data.map", DATA_LIB)
        segments_end = data_end + len(SEGMENTS_SOURCES)
        link(objs[data_end:segments_end], "exports_segments.map", SEGMENTS_LIB)
        score_end = segments_end + len(SCORE_SOURCES)
        link(objs[segments_end:score_end], "exports_score.map", SCORE_LIB)
        draws_end = score_end + len(DRAWS_SOURCES)
        link(objs[score_end:draws_end], "exports_draws.map", DRAWS_LIB)
        warp_end = draws_end + len(WARP_SOURCES)
        link(objs[draws_end:warp_end], "exports_warp.map", WARP_LIB)
        pitch_end = warp_end + len(PITCH_SOURCES)
        link(objs[warp_end:pitch_end], "exports_pitch.map", PITCH_LIB)
        link(objs[pitch_end:], "exports_soft.map", SOFT_LIB)
    return out


if __name__ == "__main__":
    build_library(force="--force" in sys.argv)
    print(LIB)
