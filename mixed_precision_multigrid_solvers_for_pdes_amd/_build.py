"""Builds libmghip.so (HIP, gfx950) in-tree with hipcc.  Cross-compiles without a GPU.

Every csrc/*.hip translation unit is compiled to an object of its own (in parallel, and only when it or a header it includes
is newer than its object), then linked.  mg_launch.hip is the one unit that instantiates the kernels of mg_kernels.hpp and
mg_rb_kernels.hpp (minutes); the engine, the solve loop and the stateless ABI are host code (seconds), so an edit there
rebuilds that unit alone.  mg_pcg.hip holds the Krylov outer loop with the kernels of mg_pcg_kernels.hpp, mg_heat.hip the time
stepper with those of mg_heat_kernels.hpp, mg_line.hip the zebra line smoothers with the kernel of mg_line_kernels.hpp, mg_eig.hip
the block eigensolver with the kernels of mg_eig_kernels.hpp (and the host-only mg_eig_dense.hpp); no other unit includes any of
these headers.  mg_ho.hip holds the fourth-order compact operator with the kernels of mg_ho_kernels.hpp; include/mghip_ho.h is
included there and by mg_pcg.hip, which defines mg_pcg_set_order.  mg_flow.hip holds the vorticity / stream-function stepper with the
kernels of mg_flow_kernels.hpp and its C header include/mghip_flow.h; no other unit includes either.  mg_nl.hip holds the
semilinear Newton method (the eval kernel of mg_nl_kernels.hpp, its launcher and the driver); include/mghip_nl.h is included there
and by mg_pcg.hip, which defines mg_pcg_set_reaction_device and calls the eval kernel's launcher through mg_host.hpp.  mg_rd.hip holds the
reaction-diffusion stepper with the kernels of mg_rd_kernels.hpp and its C header include/mghip_rd.h (which includes mghip_nl.h);
no other unit includes either, and mg_rd.hip includes no other family's kernels: the ring fill and the difference norm are the
heat stepper's exported device forms.  mg_tile.hpp holds what the kernels of the seven solver modules share (tile walk, five-point
operator, masked store, ring decode, fixed-order reduce); it is included by their seven kernel headers and by nothing else.
mg_3d.hip holds the 3-D multigrid family (the engine, its stateless device forms and the kernels of mg_3d_kernels.hpp) with its C
header include/mghip_3d.h; no other unit includes either, and mg_3d.hip includes no other family's kernels and not mg_tile.hpp: it
takes the pitch rule through the C ABI and the fixed-order reduce from mg_kernels.hpp."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
OBJDIR = os.path.join(LIBDIR, "obj")
LIBPATH = os.path.join(LIBDIR, "libmghip.so")
SOURCES = [os.path.join(CSRC, n) for n in ("mg_launch.hip", "mg_engine.hip", "mg_solve.hip", "mg_dev.hip", "mg_plan.hip", "mg_tail.hip", "mg_pcg.hip", "mg_heat.hip", "mg_line.hip", "mg_eig.hip", "mg_ho.hip", "mg_flow.hip", "mg_nl.hip", "mg_rd.hip", "mg_3d.hip")]
HEADERS = [os.path.join(CSRC, n) for n in ("mg_kernels.hpp", "mg_tile.hpp", "mg_rb_kernels.hpp", "mg_tail_kernels.hpp", "mg_host.hpp", "mg_launch.hpp", "mg_pcg_kernels.hpp",
                                               "mg_heat_kernels.hpp", "mg_line_kernels.hpp", "mg_eig_kernels.hpp", "mg_eig_dense.hpp", "mg_ho_kernels.hpp", "mg_flow_kernels.hpp", "mg_nl_kernels.hpp", "mg_rd_kernels.hpp", "mg_3d_kernels.hpp")] + \
          [os.path.join(os.path.dirname(HERE), "include", n) for n in ("mghip.h", "mghip_heat.h", "mghip_line.h", "mghip_eig.h", "mghip_ho.h", "mghip_flow.h", "mghip_nl.h", "mghip_rd.h", "mghip_3d.h")]
DEPS = SOURCES + HEADERS
# headers a unit does NOT include (directly or through another header; checked against hipcc -MM): editing them leaves its
# object current
_LINE = ("mg_line_kernels.hpp", "mghip_line.h")           # only mg_line.hip includes these
_EIG = ("mg_eig_kernels.hpp", "mg_eig_dense.hpp", "mghip_eig.h")      # only mg_eig.hip includes these
_HO = ("mg_ho_kernels.hpp", "mghip_ho.h")                 # only mg_ho.hip includes the kernels; mg_pcg.hip includes the C header too
_FLOW = ("mg_flow_kernels.hpp", "mghip_flow.h")         # only mg_flow.hip includes these
_NL = ("mg_nl_kernels.hpp", "mghip_nl.h")                 # only mg_nl.hip includes the kernel; mg_pcg.hip includes the C header too
_RD = ("mg_rd_kernels.hpp", "mghip_rd.h")                 # only mg_rd.hip includes these (and through mghip_rd.h the Newton method's C header)
_3D = ("mg_3d_kernels.hpp", "mghip_3d.h")                 # only mg_3d.hip includes these
_HOST_UNIT = ("mg_tile.hpp", "mg_rb_kernels.hpp", "mg_tail_kernels.hpp", "mg_pcg_kernels.hpp", "mg_heat_kernels.hpp") + _LINE + _EIG + _HO + _FLOW + _NL + _RD + _3D    # mg_kernels.hpp comes with mg_host.hpp (types and constants)
NOT_INCLUDED = {"mg_launch.hip": ("mg_tile.hpp", "mg_tail_kernels.hpp", "mg_pcg_kernels.hpp", "mg_heat_kernels.hpp") + _LINE + _EIG + _HO + _FLOW + _NL + _RD + _3D,
                "mg_engine.hip": _HOST_UNIT, "mg_solve.hip": _HOST_UNIT, "mg_dev.hip": _HOST_UNIT,
                "mg_tail.hip": ("mg_tile.hpp", "mg_launch.hpp", "mg_pcg_kernels.hpp", "mg_heat_kernels.hpp") + _LINE + _EIG + _HO + _FLOW + _NL + _RD + _3D,
                "mg_pcg.hip": ("mg_rb_kernels.hpp", "mg_tail_kernels.hpp", "mg_heat_kernels.hpp", "mg_ho_kernels.hpp", "mg_nl_kernels.hpp") + _LINE + _EIG + _FLOW + _RD + _3D,
                "mg_heat.hip": ("mg_rb_kernels.hpp", "mg_tail_kernels.hpp", "mg_launch.hpp", "mg_pcg_kernels.hpp") + _LINE + _EIG + _HO + _FLOW + _NL + _RD + _3D,
                "mg_line.hip": ("mg_tile.hpp", "mg_rb_kernels.hpp", "mg_tail_kernels.hpp", "mg_pcg_kernels.hpp", "mg_heat_kernels.hpp") + _EIG + _HO + _FLOW + _NL + _RD + _3D,
                "mg_eig.hip": ("mg_rb_kernels.hpp", "mg_tail_kernels.hpp", "mg_pcg_kernels.hpp", "mg_heat_kernels.hpp") + _LINE + _HO + _FLOW + _NL + _RD + _3D,
                "mg_ho.hip": ("mg_rb_kernels.hpp", "mg_tail_kernels.hpp", "mg_pcg_kernels.hpp", "mg_heat_kernels.hpp") + _LINE + _EIG + _FLOW + _NL + _RD + _3D,
                "mg_flow.hip": ("mg_rb_kernels.hpp", "mg_tail_kernels.hpp", "mg_launch.hpp", "mg_pcg_kernels.hpp", "mg_heat_kernels.hpp") + _LINE + _EIG + _HO + _NL + _RD + _3D,
                "mg_nl.hip": ("mg_rb_kernels.hpp", "mg_tail_kernels.hpp", "mg_pcg_kernels.hpp", "mg_heat_kernels.hpp") + _LINE + _EIG + _HO + _FLOW + _RD + _3D,
                "mg_plan.hip": ("mg_kernels.hpp", "mg_tile.hpp", "mg_rb_kernels.hpp", "mg_tail_kernels.hpp", "mg_host.hpp", "mg_launch.hpp",
                                "mg_pcg_kernels.hpp", "mg_heat_kernels.hpp", "mghip_heat.h") + _LINE + _EIG + _HO + _FLOW + _NL + _RD + _3D,
                "mg_rd.hip": ("mg_rb_kernels.hpp", "mg_tail_kernels.hpp", "mg_launch.hpp", "mg_pcg_kernels.hpp", "mg_heat_kernels.hpp", "mg_nl_kernels.hpp") + _LINE + _EIG + _HO + _FLOW + _3D,
                "mg_3d.hip": ("mg_tile.hpp", "mg_rb_kernels.hpp", "mg_tail_kernels.hpp", "mg_launch.hpp", "mg_pcg_kernels.hpp", "mg_heat_kernels.hpp") +
                             _LINE + _EIG + _HO + _FLOW + _NL + _RD}
# -ffp-contract=off: the kernels reproduce the reference's rounding sequence (no FMA contraction).
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]


def extra_flags():
    """MGHIP_EXTRA_FLAGS: extra compiler flags (measurement builds: -DMG_EXPERIMENTS turns the experiment switches of the
    kernels on; such a build goes to its own file through MGHIP_LIBRARY_OUT and is never the shipped library)."""
    return os.environ.get("MGHIP_EXTRA_FLAGS", "").split()


def hipcc_path():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC or install ROCm under /opt/rocm)")


def source_hash():
    """sha1 over the kernel sources (csrc/*.hip, *.hpp and the C header): which build a stored measurement belongs to"""
    import hashlib
    h = hashlib.sha1()
    for path in sorted(DEPS):
        if os.path.exists(path):
            h.update(os.path.basename(path).encode())
            h.update(open(path, "rb").read())
    return h.hexdigest()[:12]


def is_stale():
    if not os.path.exists(LIBPATH):
        return True
    t = os.path.getmtime(LIBPATH)
    return any(os.path.getmtime(d) > t for d in DEPS if os.path.exists(d))


def _obj_of(src, tag=""):
    return os.path.join(OBJDIR, os.path.splitext(os.path.basename(src))[0] + tag + ".o")


def _obj_stale(src, obj):
    if not os.path.exists(obj):
        return True
    t = os.path.getmtime(obj)
    skip = NOT_INCLUDED.get(os.path.basename(src), ())
    deps = [src] + [hd for hd in HEADERS if os.path.basename(hd) not in skip]
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build_library(force=False, verbose=False, out=None):
    """Compile csrc/*.hip -> lib/libmghip.so.  Returns the library path.

    Several ranks may import the package at once (torch.distributed.run): the build is serialised with a file
    lock and the library is written to a temporary name and renamed into place, so nobody maps a half-written file."""
    out = out or os.environ.get("MGHIP_LIBRARY_OUT") or LIBPATH
    extra = extra_flags()
    if out == LIBPATH and extra:
        raise RuntimeError("MGHIP_EXTRA_FLAGS builds are measurement builds: set MGHIP_LIBRARY_OUT to a file of their own")
    if not force and out == LIBPATH and not is_stale():
        return LIBPATH
    import fcntl
    os.makedirs(OBJDIR, exist_ok=True)
    tag = "" if out == LIBPATH else "." + os.path.splitext(os.path.basename(out))[0]
    with open(os.path.join(LIBDIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and out == LIBPATH and not is_stale():          # another process built it while we waited
                return LIBPATH
            cc = hipcc_path()
            todo = [(s, _obj_of(s, tag)) for s in SOURCES if os.path.exists(s)]

            def compile_one(pair):
                src, obj = pair
                if not force and not _obj_stale(src, obj):
                    return None
                tmp = f"{obj}.{os.getpid()}.tmp"
                cmd = [cc] + FLAGS + extra + ["-c", "-o", tmp, src]
                if verbose:
                    print(" ".join(cmd))
                res = subprocess.run(cmd, capture_output=True, text=True)
                if res.returncode != 0:
                    if os.path.exists(tmp):
                        os.remove(tmp)
                    return f"{os.path.basename(src)}:\n{res.stdout}{res.stderr}"
                os.replace(tmp, obj)
                return None
            with ThreadPoolExecutor(max_workers=max(1, min(len(todo), 16))) as pool:
                errors = [e for e in pool.map(compile_one, todo) if e]
            if errors:
                raise RuntimeError("hipcc failed:\n" + "\n".join(errors))
            tmp = f"{out}.{os.getpid()}.tmp"
            cmd = [cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + [o for _, o in todo]
            if verbose:
                print(" ".join(cmd))
            res = subprocess.run(cmd, capture_output=True, text=True)
            if res.returncode != 0:
                if os.path.exists(tmp):
                    os.remove(tmp)
                raise RuntimeError("hipcc (link) failed:\n" + res.stdout + res.stderr)
            os.replace(tmp, out)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return out


if __name__ == "__main__":
    print(build_library(force=True, verbose=True))
