"""Builds libe3dge_hip.so (gfx950) in-tree with hipcc.  No torch headers are involved: the library is a
plain C-ABI shared object (include/e3dge_hip.h) loaded with ctypes."""
import hashlib
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIBNAME = "libe3dge_hip.so"
SOURCES = ["stream_ops.hip", "upfirdn2d.hip", "siren.hip", "siren_bwd.hip", "resblock.hip", "modconv.hip", "decoder2.hip", "local_query.hip", "metrics.hip", "align_volume.hip", "hitprob.hip", "siren_ws.hip", "wgrad.hip",
           "marching_cubes.hip", "mesh_render.hip", "lpips.hip", "idnet.hip", "losses.hip", "disc.hip", "hgfilter.hip", "aligner.hip", "volume_disc.hip"]
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-ffp-contract=on", "-fno-slp-vectorize",
         "-Wno-unused-result"]  # no SLP: packed-f32 VALU next to MFMAs is slower and un-does the epilogue interleave


def lib_path():
    return os.path.join(LIBDIR, LIBNAME)


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC=...)")


def _digest():
    h = hashlib.sha256()
    for name in sorted(os.listdir(CSRC)) + ["../../include/e3dge_hip.h"]:
        with open(os.path.join(CSRC, name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    h.update(" ".join(FLAGS).encode())
    return h.hexdigest()


def _compile(pairs, flags, verbose, jobs):
    """hipcc -c for every (source name, object path) of `pairs`, at most `jobs` at a time."""
    hipcc = _hipcc()
    todo, running = list(pairs), []
    while todo or running:
        while todo and len(running) < jobs:
            src, obj = todo.pop(0)
            cmd = [hipcc, *flags, "-c", os.path.join(CSRC, src), "-o", obj]
            if verbose:
                print("[e3dge build]", " ".join(cmd), flush=True)
            running.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        src, p = running.pop(0)
        out, _ = p.communicate()
        if p.returncode != 0:
            for _, q in running:
                q.kill()
            raise RuntimeError(f"hipcc failed on {src}:\n{out}")
        if verbose and out.strip():
            print(out)


def _link(objs, target, verbose):
    cmd = [_hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", *objs, "-o", target]
    if verbose:
        print("[e3dge build]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return target


def _obj(src, prefix=""):
    return os.path.join(LIBDIR, prefix + src.replace(".hip", ".o"))


def build(force=False, verbose=True):
    """Compile every .hip source for gfx950 and link the shared library.  Returns its path."""
    os.makedirs(LIBDIR, exist_ok=True)
    stamp = os.path.join(LIBDIR, ".build_digest")
    dig = _digest()
    if not force and os.path.exists(lib_path()) and os.path.exists(stamp) and open(stamp).read() == dig:
        return lib_path()
    _compile([(src, _obj(src)) for src in SOURCES], FLAGS, verbose, jobs=len(SOURCES))
    _link([_obj(src) for src in SOURCES], lib_path(), verbose)
    with open(stamp, "w") as f:
        f.write(dig)
    return lib_path()


def build_variant(name, defines=(), only=None, verbose=True):
    """lib/variants/lib_<name>.so: the same sources and flags plus `defines` ("-DX=1", ...), for instrumented and A/B builds (load it
    with E3DGE_LIB_PATH).  only="siren_bwd": recompile that one source and link the default build's objects of the others (lib/*.o, so
    build() must have run here): seconds instead of minutes."""
    vdir = os.path.join(LIBDIR, "variants")
    os.makedirs(vdir, exist_ok=True)
    if only is not None and only + ".hip" not in SOURCES:
        raise ValueError(f"{only}.hip is not one of the library's sources")
    mine = [src for src in SOURCES if only is None or src == only + ".hip"]
    tmp = {src: os.path.join(vdir, f"{name}_" + src.replace(".hip", ".o")) for src in mine}
    try:
        _compile(list(tmp.items()), [*FLAGS, *defines], verbose, jobs=min(16, os.cpu_count() or 1))
        return _link([tmp.get(src, _obj(src)) for src in SOURCES], os.path.join(vdir, f"lib_{name}.so"), verbose)
    finally:
        for obj in tmp.values():
            if os.path.exists(obj):
                os.remove(obj)


if __name__ == "__main__":     # build.py [--force]  |  build.py --variant NAME [--only STEM] [-DFLAG=..]...
    argv = sys.argv[1:]
    if "--variant" in argv:
        name = argv[argv.index("--variant") + 1]
        only = argv[argv.index("--only") + 1] if "--only" in argv else None
        print(build_variant(name, [a for a in argv if a.startswith("-D")], only))
    else:
        print(build(force="--force" in argv))
