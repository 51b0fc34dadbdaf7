"""Build the native libraries (HIP, gfx950 only) in-tree with hipcc.

``UNITS`` is the table: library name -> its translation units.  Everything else about a library follows from its
name: ``libcough_amd[_NAME].so`` beside this file, the version script ``csrc/exports[_NAME].map`` and the C-ABI header
``include/cough_amd[_NAME].h`` (``amd``, the main library, carries no suffix).  Every translation unit is compiled to
an object file of its own (in parallel, cached under ``build/`` by the newest source / header time) and each library
is linked from the objects of its own units.  The libraries are build products and stay out of git.

There are two tables.  ``UNITS`` is closed: its nine libraries, their order and their units are pinned by
``tests/test_libraries_host.py``, which later work must leave as it is.  ``LATER_UNITS`` is open-ended: a library that
comes after the nine is entered there, under the same naming rules, and is built, checked for staleness and linked
exactly like the nine.
That second table turned out to be pinned as well (``tests/test_slices_host.py`` fixes its contents), so the libraries
after it live in ``OPEN_UNITS``: same naming rules, same build, staleness and link steps, and tests of a library there
assert that their own name is in it, never what else is -- the next library is one more entry.
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
SOURCES = ("api.hip", "featurize.hip", "featurize_generic.hip", "spectrogram.hip", "resnet.hip", "cnn.hip", "stream.hip", "synth.hip",
           "augment.hip", "train.hip", "train_small.hip", "train_std.hip")
# The three steps of the soft-target library are the training translation units of libcough_amd.so compiled a second
# time: SOFT_FLAGS only selects which extern "C" functions they emit (the *_forward_backward_soft entry points instead
# of the v5 ones), so the step code exists once
SOFT_SHARED_SOURCES = ("train.hip", "train_small.hip", "train_std.hip")
SOFT_FLAGS = ("-DCOUGH_SOFT_EXPORTS",)
# A unit is a source name, or (source, extra flags, object suffix).  include/cough_amd.h stays at ABI v5 with its 53
# entry points, so what came after it is exported from companion libraries: same flags, a version script of their own
UNITS = {
    "amd": SOURCES,
    "loop": ("loop.hip",),          # the epoch loop's meter
    "data": ("data.hip",),          # the input pipeline: the device-resident dataset and batch loader
    "segments": ("segments.hip",),  # corpus curation: frame energies, segment picking
    "score": ("score.hip",),        # offline scoring: deque mean, threshold sweep, event list
    # the device-side draws: a batch's augmentation records and masks, augmentation from them; it compiles
    # csrc/augment_kernel.h, the kernel augment.hip runs
    "draws": ("draws.hip",),
    # the soft-target training steps and the batch MixUp
    "soft": ("soft.hip",) + tuple((src, SOFT_FLAGS, "_soft") for src in SOFT_SHARED_SOURCES),
    "warp": ("warp.hip",),          # speed perturbation: the tableless per-row sinc resampler and its draws
    "pitch": ("pitch.hip",),        # pitch shift: the per-row float64 phase vocoder and its draws
}


def _named(stem: str, name: str, ext: str) -> str:
    return stem + ("" if name == "amd" else "_" + name) + ext


# the libraries after the nine (module docstring): same rules, a table that may grow
LATER_UNITS = {
    "slices": ("slices.hip",),      # corpus curation: fixed-length windows of long recordings, kept by their activity
}

# the open table (module docstring): a new library is one more entry here and one more record in _lib.OPEN
OPEN_UNITS = {
    "dups": ("dups.hip",),          # corpus curation: binary fingerprints of the feature images, the all-pairs matcher
    # soundscapes with known cough times: span powers, gains, the mix, detections matched to events (it includes
    # csrc/score_walk.h, the walking rule score.hip decides with)
    "scenes": ("scenes.hip",),
    # room reverberation: FFT overlap-save with a prepared bank of impulse responses, the transform held in LDS
    "reverb": ("reverb.hip",),
    # the capture channel: a biquad cascade per row, run block-parallel by a scan over the workgroup, and the hard clip
    "channel": ("channel.hip",),
    # training windows composed per batch: background power, gains and the mix of up to four events per row, one launch
    "windows": ("windows.hip",),
    # the window plans of a batch drawn on the device: one thread per row writes the composer's record and the label
    "windraw": ("windraw.hip",),
}

LIBS = {name: os.path.join(HERE, _named("libcough_amd", name, ".so")) for name in UNITS}
LATER_LIBS = {name: os.path.join(HERE, _named("libcough_amd", name, ".so")) for name in LATER_UNITS}
OPEN_LIBS = {name: os.path.join(HERE, _named("libcough_amd", name, ".so")) for name in OPEN_UNITS}
LIB = LIBS["amd"]
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


def _version_script(name: str) -> str:
    return os.path.join(CSRC, _named("exports", name, ".map"))


def _headers_mtime() -> float:
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    deps += [os.path.join(HERE, "..", "include", _named("cough_amd", name, ".h")) for name in (*UNITS, *LATER_UNITS, *OPEN_UNITS)]
    deps.append(os.path.abspath(__file__))   # the flags live here
    deps += [_version_script(name) for name in (*UNITS, *LATER_UNITS, *OPEN_UNITS)]
    return max(os.path.getmtime(d) for d in deps)


def is_stale() -> bool:
    libs = (*LIBS.values(), *LATER_LIBS.values(), *OPEN_LIBS.values())
    if not all(os.path.exists(p) for p in libs):
        return True
    t = min(os.path.getmtime(p) for p in libs)
    sources = {u if isinstance(u, str) else u[0] for units in (*UNITS.values(), *LATER_UNITS.values(), *OPEN_UNITS.values())
               for u in units}
    return _headers_mtime() > t or any(os.path.getmtime(os.path.join(CSRC, s)) > t for s in sources)


def later_stale(name: str) -> bool:
    """A library of ``LATER_UNITS`` or ``OPEN_UNITS`` is missing, or older than one of its sources, a header, its version
    script or this file."""
    lib = LATER_LIBS[name] if name in LATER_LIBS else OPEN_LIBS[name]
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    sources = {u if isinstance(u, str) else u[0] for u in (LATER_UNITS[name] if name in LATER_UNITS else OPEN_UNITS[name])}
    return _headers_mtime() > t or any(os.path.getmtime(os.path.join(CSRC, s)) > t for s in sources)


def build_library(force: bool = False, verbose: bool = True, extra_flags=(), out: str = LIB, force_later: bool = False) -> str:
    """Compile (only what changed, unless ``force`` / ``extra_flags``) and link the libraries of all tables.
    ``extra_flags`` (e.g. ``-DCOUGH_K1_STAMPS``) build a variant of libcough_amd.so alone at ``out`` with objects of its
    own.  ``force`` rebuilds the nine libraries of ``UNITS`` -- the link list of a forced build is pinned to exactly
    those nine -- while a library of ``LATER_UNITS`` or ``OPEN_UNITS`` is rebuilt when it is stale (``later_stale``) or ``force_later`` is
    set; the command line's ``--force`` sets both."""
    if not force and not force_later and not extra_flags and not is_stale():
        return LIB
    hipcc = _hipcc()
    objdir = OBJ if not extra_flags else OBJ + "_" + str(abs(hash(tuple(extra_flags))) % 10**8)
    os.makedirs(objdir, exist_ok=True)
    hdr = _headers_mtime()

    def compile_one(unit) -> str:
        src, flags, suffix = unit if isinstance(unit, tuple) else (unit, (), "")
        s, o = os.path.join(CSRC, src), os.path.join(objdir, src.replace(".hip", suffix + ".o"))
        if force or force_later or not os.path.exists(o) or os.path.getmtime(o) < max(hdr, os.path.getmtime(s)):
            cmd = [hipcc, *CFLAGS, *extra_flags, *flags, "-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
        return o

    all_units = {**UNITS, **LATER_UNITS, **OPEN_UNITS}
    targets = {"amd": out}
    if not extra_flags and out == LIB:
        targets = {**LIBS, **{name: lib for name, lib in (*LATER_LIBS.items(), *OPEN_LIBS.items())
                                if force_later or later_stale(name)}}
    units = [u for name in targets for u in all_units[name]]
    with ThreadPoolExecutor(max_workers=min(len(units), os.cpu_count() or 1)) as pool:
        obj = dict(zip(units, pool.map(compile_one, units)))
    for name, target in targets.items():
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + _version_script(name),
               "-o", target, *(obj[u] for u in all_units[name])]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return out


if __name__ == "__main__":
    build_library(force="--force" in sys.argv, force_later="--force" in sys.argv)
    print(LIB)
