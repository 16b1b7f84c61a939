"""Build laenerf_amd/lib/liblaenerf_hip.so (HIP kernels + C ABI) for gfx950 with hipcc.

hipcc cross-compiles without a GPU; the resulting .so is kept in-tree (git-ignored) so it
travels to the GPU box with the snapshot.  `python -m laenerf_amd.build [--force]`.

Device code is compiled WITHOUT gfx950's packed-fp32 instructions (round 5; the erratum note below) and goes through its
assembly: every .hip file's device half is compiled to gfx950 assembly with `-target-feature -packed-fp32-ops`, the assembly is
checked (no v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 / v_pk_mov_b32 may be left), assembled / linked / bundled with the LLVM
tools of the ROCm image, and the host half of the file is compiled against that code object (`-fcuda-include-gpubinary`) -- the
steps `hipcc -c` runs internally, with the device half's own flags and one check in between.
"""
import concurrent.futures
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
SO = os.path.join(LIBDIR, "liblaenerf_hip.so")
SOURCES = ["raymarching.hip", "frame.hip", "gridencoder.hip", "gridbackward.hip", "shencoder.hip", "freqencoder.hip", "ffmlp.hip", "nerfhead.hip", "mlpbackward.hip", "densitygrid.hip", "optimizer.hip", "loss.hip", "palette.hip", "editgrid.hip", "masklift.hip", "region.hip", "insert.hip", "tsdf.hip", "atlas.hip", "simplify.hip", "undistort.hip", "batch.hip", "recolor.hip", "style_batch.hip", "style_image.hip", "distill.hip", "mesh.hip", "components.hip", "evaluate.hip", "ssim.hip", "nnfm.hip", "rayreg.hip", "ref_stage.hip", "pose.hip", "exposure.hip", "lae_common.cpp"]
# -ffp-contract=off: only explicit fmaf() fuses -> bit-identical sample indices/positions vs the oracle
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
         "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
         # MFMA accumulators in VGPRs: with the default AGPR form every accumulator tile is copied back with
         # v_accvgpr_read before the VALU epilogue (88 copies per 16-row tile in the fused head, 1036 -> 940 instructions)
         "-mllvm", "-amdgpu-mfma-vgpr-form=1"]
LLVM_BIN = os.environ.get("LAE_LLVM_BIN", "/opt/rocm/lib/llvm/bin")

# ---------------------------------------------------------------------------------------------------------------------------
# gfx950 packed-fp32 operand-selection erratum (found in round 5; DESIGN.md section 8a, tools/ubench/pk_opsel.hip,
# profiles/r5_pk_opsel_erratum.txt, profiles/r5_suite_beside_mfma.txt).  While v_mfma instructions of ANOTHER wave are in flight
# on the SIMD (a kernel on a second stream, or a second process on the GPU), a packed-fp32 instruction whose LOW result takes the
# HIGH half of SRC1 (op_sel = [0,1,..]) with SRC1 in VGPRs can compute that result with SRC1.hi read as ZERO: v_pk_mul_f32 /
# v_pk_add_f32 in 0.06-10 % of the instructions of an isolated test, v_pk_fma_f32 in lanes 48-63 of EVERY wave of k_grid_fwd's
# dy_dx chain (11 parity tests fail beside an MFMA-spinning process, every time).  The compiler emits such forms wherever it folds
# a lane shuffle into a packed operation.  Which forms are safe could only be established empirically, so none is used: the
# device half is compiled with the `packed-fp32-ops` target feature off (same-box A/B of the bench: train step 0.352 against
# 0.355 ms, frames equal, style step +3 % -- nothing to lose).  LAE_BUILD_PACKED_FP32=1 / --packed-fp32 turn the feature back on
# for the reproducers (tools/grid_loop_fault.sh, tools/mfma_neighbour_check.py --lib ...).
NO_PACKED_FP32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]      # device half only (x86 does not know the feature)
_PK_FP32 = re.compile(r"^\s*v_pk_(?:mul_f32|add_f32|fma_f32|mov_b32)\b")


def packed_fp32_instructions(asm_text):
    """the packed-fp32 instructions of a piece of gfx950 assembly / disassembly (lines)"""
    return [ln.strip() for ln in asm_text.split("\n") if _PK_FP32.match(ln.split(";")[0].split("//")[0])]


def _deps():
    out = [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    out.append(os.path.join(HERE, "..", "include", "laenerf.h"))
    out.append(os.path.abspath(__file__))
    return out


def needs_build():
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    return any(os.path.getmtime(d) > t for d in _deps())


def build(force=False, verbose=False, out=None, extra_flags=(), packed_fp32=False):
    """out / extra_flags / packed_fp32=True: probe builds (tools/grid_loop_fault.sh) -- another library file, never the in-tree
    default: packed_fp32 and LAE_BUILD_PACKED_FP32=1 are honoured only together with `out` (a default library built
    with them would be newer than its sources and be loaded silently ever after).  The target path is an argument of _build,
    not a module global: a probe build can run beside an automatic rebuild of the default library."""
    want_packed = bool(packed_fp32) or os.environ.get("LAE_BUILD_PACKED_FP32") == "1"
    if out is not None:
        target = os.path.abspath(out)
        if os.path.realpath(target) == os.path.realpath(SO) and want_packed:
            raise RuntimeError("laenerf_amd.build: the packed-fp32 probe build must not replace the default library; pick another --out")
        os.makedirs(os.path.dirname(target), exist_ok=True)
        return _build(verbose, list(extra_flags), want_packed, target)
    if want_packed:
        raise RuntimeError("laenerf_amd.build: packed_fp32 / LAE_BUILD_PACKED_FP32=1 need out=<another library file> "
                           "(`python -m laenerf_amd.build --out lib.so --packed-fp32`); the default library never has packed-fp32 code")
    if not force and not needs_build() and not default_is_packed():
        return SO
    return _build(verbose, [], False, SO)


def default_is_packed(so=None):
    """True when the record next to the (default) library says it was built WITH packed-fp32 instructions"""
    try:
        return bool(json.load(open((so or SO) + ".isa.json")).get("packed_fp32_ops"))
    except (OSError, ValueError):
        return False


def _run(cmd, verbose, what):
    if verbose:
        print(" ".join(cmd))
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if p.returncode != 0:
        sys.stderr.write(p.stdout.decode())
        raise RuntimeError(f"{what} failed")
    if verbose and p.stdout:
        print(p.stdout.decode())


def _compile_one(src, obj, flags, verbose, packed_fp32):
    """one translation unit: device assembly (packed fp32 off) -> check -> code object -> fat binary -> host object.
    -> packed-fp32 instructions in the device code (0 unless packed_fp32)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    path = os.path.join(CSRC, src)
    stem = obj[:-2]
    asm, dev_o, co, fb = stem + ".s", stem + ".dev.o", stem + ".co", stem + ".hipfb"
    try:
        _run([hipcc] + flags + ([] if packed_fp32 else NO_PACKED_FP32) + ["-x", "hip", "--cuda-device-only", "-S", path, "-o", asm], verbose,
             f"hipcc (device) on {src}")
        left = packed_fp32_instructions(open(asm).read())
        if left and not packed_fp32:
            raise RuntimeError(f"{src}: {len(left)} packed-fp32 instruction(s) in the device code although the feature is off: {left[:3]}")
        _run([os.path.join(LLVM_BIN, "clang"), "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950", "-c", asm, "-o", dev_o], verbose, f"assembler on {src}")
        _run([os.path.join(LLVM_BIN, "lld"), "-flavor", "gnu", "-m", "elf64_amdgpu", "--no-undefined", "-shared", "-o", co, dev_o], verbose, f"lld on {src}")
        _run([os.path.join(LLVM_BIN, "clang-offload-bundler"), "-type=o", "-bundle-align=4096",
              "-targets=host-x86_64-unknown-linux-gnu,hipv4-amdgcn-amd-amdhsa--gfx950", "-input=/dev/null", f"-input={co}", f"-output={fb}"], verbose, f"bundler on {src}")
        _run([hipcc] + flags + ["-x", "hip", "--cuda-host-only", "-Xclang", "-fcuda-include-gpubinary", "-Xclang", fb, "-c", path, "-o", obj], verbose, f"hipcc (host) on {src}")
        return len(left)
    finally:
        for f in (asm, dev_o, co, fb):
            if os.path.exists(f):
                os.remove(f)


def _build(verbose, more, packed_fp32, SO):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = os.environ.get("LAE_BUILD_EXTRA_FLAGS", "").split() + more      # probes only (e.g. -DLAE_GRID_STAMPS, tools/grid_bwd_stamps.py)
    os.makedirs(LIBDIR, exist_ok=True)
    tag = f"{os.getpid()}.{abs(hash(SO)) % 100000}"                         # per-process, per-target object names: concurrent builds do not share files
    objs = [os.path.join(LIBDIR, f"{src.rsplit('.', 1)[0]}.{tag}.o") for src in SOURCES]
    counts = {}
    try:
        with concurrent.futures.ThreadPoolExecutor(len(SOURCES)) as ex:
            futs = {src: ex.submit(_compile_one, src, obj, FLAGS + extra, verbose, packed_fp32) for src, obj in zip(SOURCES, objs)}
            for src, f in futs.items():
                counts[src] = f.result()
        tmp_so = SO + f".{os.getpid()}.tmp"                      # link to a temp name, then rename: a reader never maps a half-written library
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp_so] + objs)
        os.replace(tmp_so, SO)
        with open(SO + ".isa.json", "w") as f:
            json.dump({"packed_fp32_ops": bool(packed_fp32), "packed_fp32_instructions": counts, "total": sum(counts.values())}, f)
    finally:
        for o in objs:
            if os.path.exists(o):
                os.remove(o)
    return SO


if __name__ == "__main__":
    if "--out" in sys.argv:                                  # python -m laenerf_amd.build --out path.so [-DFLAG ...] [--packed-fp32]
        print(build(out=sys.argv[sys.argv.index("--out") + 1], extra_flags=[a for a in sys.argv[1:] if a.startswith("-D")], verbose=True,
                    packed_fp32="--packed-fp32" in sys.argv))
    else:
        print(build(force="--force" in sys.argv, verbose=True))
