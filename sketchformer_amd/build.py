"""Builds libskf.so (the C-ABI HIP library) in-tree with hipcc for gfx950."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libskf.so")
SOURCES = ["skf_model.hip", "skf_model_prof.hip", "skf_model_layout.hip", "skf_model_sched.hip", "skf_model_fwd.hip", "skf_model_bwd.hip",
           "skf_model_decode.hip", "skf_model_bf16.hip", "skf_gemm.hip", "skf_gemm_ws.hip", "skf_gemm_small.hip", "skf_gemm_wsx.hip", "skf_gemm_wgrad.hip", "skf_ffn_fused.hip", "skf_attention.hip", "skf_attention_bwd2.hip", "skf_attention_bwd3.hip", "skf_rowops.hip", "skf_continuous.hip", "skf_optimizer.hip", "skf_decode.hip", "skf_decode_fused.hip", "skf_beam.hip", "skf_row_blocks.hip", "skf_generic.hip", "skf_bf16_gemm.hip", "skf_bf16_attention.hip", "skf_bf16_rowops.hip", "skf_retrieval.hip", "skf_kmeans.hip", "skf_interp.hip", "skf_tsne.hip", "skf_raster.hip", "skf_tokenize.hip", "skf_align.hip", "skf_augment.hip", "skf_simplify.hip", "skf_ragged.hip", "skf_score.hip", "skf_chamfer.hip", "skf_resample.hip", "skf_strokes.hip", "skf_flatten.hip", "skf_gradnorm.hip", "skf_accum.hip", "skf_ema.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
         # f32-input MFMA shares the VALU pipe on gfx950 (tools/micro/mfma_valu_overlap.hip): keep accumulators in VGPRs so
         # the epilogues need no v_accvgpr_read/write moves (they were ~30 % of the VALU instructions of the attention loops)
         "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-Wall", "-Wno-unused-function", "-Wno-unused-value"]
FLAGS += os.environ.get("SKF_EXTRA_HIPCC_FLAGS", "").split()   # extra compiler flags for a variant build (tools/build_variant.sh)
# per-source additions.  skf_kmeans.hip: its distance loop is scalar fp32 on purpose; left alone, -O3 pairs the
# subtracts / multiplies / fmas of neighbouring points into v_pk_*_f32, which run at the scalar rate on gfx950 and cost extra
# v_mov / s_nop around them
# skf_tokenize.hip: bit-equal to the host tokenizers: no multiply and add may be fused there
# skf_align.hip: the DTW cells are bit-equal to a float32 host restatement, for the same reason
# skf_augment.hip: bit-equal to the host augmentation: scale, then merge, each rounded on its own
# skf_simplify.hip: bit-equal to the host restatement of the RDP rule: every fp64 operation rounded on its own
# skf_chamfer.hip: bit-equal to the float32 host restatement of the shape-distance rule; its walk is scalar
# fp32 for the reason given for skf_kmeans.hip
# skf_resample.hip: bit-equal to the host restatement of the resampling rule: the fp32 length and the fp64
# interpolation are rounded operation by operation
# skf_strokes.hip: bit-equal to the host restatement of the stroke-edit rule: fp32 sums and differences only,
# held to the same setting as its neighbours
# skf_flatten.hip: bit-equal to the host restatement of the path-flattening rule: the fp64 piece count and
# the de Casteljau lerps are rounded operation by operation
# skf_gradnorm.hip: the clip scales c / max(norm, c) and the in-place x * s_e are bit-equal to the float32 restatement
# (DESIGN.md section 3w): no multiply may fuse into an add
# skf_ema.hip: shadow -= (shadow - w) * (1 - d) is bit-equal to TensorFlow's assign_moving_average and to the float32 restatement
# (DESIGN.md section 3y): the multiply must not fuse into the subtract behind it
SOURCE_FLAGS = {"skf_kmeans.hip": ["-fno-slp-vectorize"], "skf_tokenize.hip": ["-ffp-contract=off"], "skf_align.hip": ["-ffp-contract=off"],
                "skf_augment.hip": ["-ffp-contract=off"], "skf_simplify.hip": ["-ffp-contract=off"],
                "skf_chamfer.hip": ["-ffp-contract=off", "-fno-slp-vectorize"], "skf_resample.hip": ["-ffp-contract=off"],
                "skf_strokes.hip": ["-ffp-contract=off"], "skf_flatten.hip": ["-ffp-contract=off"], "skf_gradnorm.hip": ["-ffp-contract=off"],
                "skf_ema.hip": ["-ffp-contract=off"]}


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


STAMP = LIB + ".stamp"


def _source_digest():
    """sha256 over every file the library is built from + the compiler flags (file times do not survive a snapshot copy)."""
    import hashlib
    h = hashlib.sha256((" ".join(FLAGS) + repr(sorted(SOURCE_FLAGS.items()))).encode())
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC)) + [os.path.join(HERE, "..", "include", "skf.h")]
    for path in files:
        h.update(os.path.basename(path).encode())
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def needs_build():
    if not os.path.exists(LIB) or not os.path.exists(STAMP):
        return True
    with open(STAMP) as f:
        return f.read().strip() != _source_digest()


def build_library(force=False, verbose=True):
    """Compile every HIP source for gfx950 and link libskf.so next to this file."""
    if not force and not needs_build():
        return LIB
    objs = []
    procs = []
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    for src in SOURCES:
        obj = os.path.join(HERE, "build", src.replace(".hip", ".o"))
        cmd = [_hipcc()] + FLAGS + SOURCE_FLAGS.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        objs.append(obj)
    failed = False
    for src, p in procs:
        out, _ = p.communicate()
        if out and verbose:
            sys.stdout.write(out.decode(errors="replace"))
        if p.returncode != 0:
            failed = True
            sys.stderr.write("hipcc failed on %s\n%s\n" % (src, out.decode(errors="replace")))
    if failed:
        raise RuntimeError("libskf.so build failed")
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(STAMP, "w") as f:
        f.write(_source_digest())
    return LIB


if __name__ == "__main__":
    build_library(force="--force" in sys.argv)
    print(LIB)
