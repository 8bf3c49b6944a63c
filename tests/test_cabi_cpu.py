"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and
exports every symbol include/skf.h declares (no compute calls without a GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from sketchformer_amd import build, _lib
    build.build_library(verbose=False)
    return _lib.load()


def _declared():
    text = open(os.path.join(ROOT, "include", "skf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(skf_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported(lib):
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), "libskf.so does not export %s" % n


def test_binding_table_matches_header(lib):
    from sketchformer_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared()


_CTYPE_OF = {"int32_t": "c_int32", "uint32_t": "c_uint32", "float": "c_float", "int64_t": "c_int64", "char": "c_char"}


def _header_struct_fields(name):
    """[(field, ctypes type name)] of `typedef struct <name> {...}` as include/skf.h declares it, in order."""
    text = open(os.path.join(ROOT, "include", "skf.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.*)$", decl, flags=re.S)
        ctype, star, names = m.group(1), m.group(2), m.group(3)
        for n in names.split(","):
            n = n.strip()
            arr = re.match(r"(\w+)\[(\d+)\]$", n)
            if arr:
                out.append((arr.group(1), "%s*%s" % (_CTYPE_OF[ctype], arr.group(2))))
            else:
                out.append((n.lstrip("*").strip(), "c_void_p" if (star or n.startswith("*")) else _CTYPE_OF[ctype]))
    return out


def _canon(pairs):
    """(field, type name) -> (field, ctypes type object) so that aliases (c_int32 is c_int) compare equal"""
    out = []
    for n, t in pairs:
        if "*" in t:
            base, length = t.split("*")
            out.append((n, (getattr(C, base), int(length))))
        else:
            out.append((n, getattr(C, t)))
    return out


def _ctypes_fields(struct):
    return [(n, (t._type_, t._length_) if hasattr(t, "_length_") else t) for n, t in struct._fields_]


def test_config_struct_layout_matches_header_binding_and_integration_doc(lib):
    """Field for field, in order: include/skf.h == sketchformer_amd/_lib.py == the binding INTEGRATION.md shows a maintainer
    (round 3's document was two fields short: a struct copied from it handed the library heap garbage)."""
    from sketchformer_amd import _lib
    header = _header_struct_fields("SkfConfig")
    assert header[0] == ("struct_size", "c_uint32") and len(header) >= 35
    assert _ctypes_fields(_lib.SkfConfig) == _canon(header)
    assert C.sizeof(_lib.SkfConfig) == lib.skf_config_size() == 4 * len(header)
    assert _ctypes_fields(_lib.SkfParamEntry) == _canon(_header_struct_fields("SkfParamEntry"))
    # the descriptor arrays that the batched reduction / weight-cast launches read from device memory
    for name, nbytes in (("SkfReduceDesc", 48), ("SkfCastDesc", 56)):
        fields = _header_struct_fields(name)
        assert _ctypes_fields(getattr(_lib, name)) == _canon(fields), name
        assert C.sizeof(getattr(_lib, name)) == nbytes == 8 * 3 + 4 * (len(fields) - 3), name
    # the `_fields_ = [...]` block of its SkfConfig
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = re.search(r"class SkfConfig\(C\.Structure\):.*?_fields_ = \[(.*?)\n    \]", doc, flags=re.S).group(1)
    doc_fields = re.findall(r'\("(\w+)",\s*C\.(c_\w+)\)', block)
    assert _canon(doc_fields) == _canon(header)
    assert "struct_size=C.sizeof(SkfConfig)" in doc


def test_config_struct_size_guard(lib):
    """A config whose struct_size is not the library's sizeof(SkfConfig) is refused by every entry that takes one."""
    from sketchformer_amd import engine
    cfg = engine.make_config(batch=4)
    assert cfg.struct_size == C.sizeof(type(cfg)) and lib.skf_config_validate(C.byref(cfg)) == 0
    for bad in (0, cfg.struct_size - 8, cfg.struct_size + 4):
        cfg.struct_size = bad
        assert lib.skf_config_validate(C.byref(cfg)) == -1
        assert b"struct_size" in lib.skf_last_error()
        assert lib.skf_model_param_floats(C.byref(cfg)) == 0 and lib.skf_model_workspace_bytes(C.byref(cfg)) == 0
        h = C.c_void_p()
        assert lib.skf_model_create(C.byref(cfg), C.byref(h)) == -1 and not h.value


def test_shipped_library_reads_no_environment():
    """include/skf.h: 'no global state'.  No source of the library calls getenv, turns a string into a device pointer or names the
    knob reader / measurement build that once did (there is one build of the library), and the library does not import getenv."""
    import glob
    import subprocess
    csrc = os.path.join(ROOT, "sketchformer_amd", "csrc")
    paths = glob.glob(os.path.join(csrc, "*"))
    assert len(paths) > 30
    for path in paths:
        text = open(path, encoding="utf-8").read()
        for gone in ("getenv(", "strtoull(", "skf_knob", "SKF_MEASURE"):
            assert gone not in text, "%s: %s" % (path, gone)
    syms = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(ROOT, "sketchformer_amd", "libskf.so")],
                          capture_output=True, text=True, check=True).stdout
    assert not re.search(r"\bU (secure_)?getenv\b", syms), "libskf.so imports getenv"


def test_kernel_parameter_blocks_have_no_diagnostic_members():
    """AttnParams / GemmParams carry operands and shapes only: no `ablate` / `dbg` member for a shipped kernel to branch on."""
    csrc = os.path.join(ROOT, "sketchformer_amd", "csrc")
    for name in ("skf_attention_params.h", "skf_gemm_params.h"):
        text = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, name), encoding="utf-8").read())
        assert re.search(r"struct (AttnParams|GemmParams) \{", text), name
        m = re.search(r"\b(ablate|dbg)\b\s*[;,=\[]", text)
        assert m is None, "%s declares %s" % (name, m.group(1))


def test_library_sources_have_no_build_time_switch():
    """No #if / #ifdef / #ifndef / #elif on an SKF_ name in csrc/ (the headers use #pragma once): one build, no -D experiments."""
    import glob
    csrc = os.path.join(ROOT, "sketchformer_amd", "csrc")
    paths = glob.glob(os.path.join(csrc, "*"))
    assert len(paths) > 30
    for path in paths:
        for ln in open(path, encoding="utf-8").read().splitlines():
            assert not re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b.*\bSKF_", ln), "%s: %s" % (path, ln.strip())


_RETIRED_KNOBS = (
    "SKF_EVLOG", "SKF_TWO_GRAD_SETS", "SKF_NO_EMBED_SORT", "SKF_NO_WAIT_DEDUPE", "SKF_EVENT_SCOPE", "SKF_NO_LN_FUSE",
    "SKF_NO_RELU_BITS", "SKF_NO_STOP_EVENTS", "SKF_TAIL_REDUCE_SIDE", "SKF_NO_DEFERRED_DGRAD", "SKF_NO_FFN_FUSE",
    "SKF_NO_FFN_CHAIN", "SKF_NO_FFN_PRE", "SKF_ATTN_ORDER", "SKF_KV_WAIT_ALL", "SKF_NO_TAIL_PROJ", "SKF_NO_FFN_LN_BWD",
    "SKF_NO_LN_DGRAD", "SKF_NO_LN_LEAD", "SKF_NO_ROW_BLOCKS", "SKF_NO_WGRAD_HOLD", "SKF_NO_BOTT_PARTIALS", "SKF_NO_EARLY_TAIL",
    "SKF_TAIL_WGRAD_SIDE", "SKF_MID_FLUSH", "SKF_DECODE_GRAPH", "SKF_NO_STAGE_KERNEL", "SKF_NO_STAGED_MASKS",
    "SKF_NO_SIDE_STREAM", "SKF_NO_SIDE_PREAMBLE",
    "SKF_GEMM_NO_SMALL", "SKF_GEMM_NO_WGRAD", "SKF_NO_WGRAD_GROUP", "SKF_GEMM_NO_WS", "SKF_NO_MASKED_CHAIN", "SKF_LN_V4",
    # the kernels' and launchers' environment knobs ...
    "SKF_ATTN_XCD", "SKF_ATTN_ABLATE", "SKF_ATTN_DBG", "SKF_ATTN_BWD2", "SKF_ATTN_BWD3", "SKF_ATTN_SPLIT", "SKF_GEMM_DBG", "SKF_GEMM_ABLATE",
    "SKF_WS_XCD", "SKF_WS_WGS", "SKF_WGRAD_WGS", "SKF_PROF_FINE", "SKF_WSX_KSPLIT", "SKF_WSX_KSPLIT256", "SKF_WSX_KSPLIT384",
    "SKF_BF16_GEMM_TILE", "SKF_BF16_GEMM_DMA", "SKF_BF16_GEMM_PH8",
    # ... and their -D names and stamp macros
    "SKF_MEASURE", "SKF_WGRAD_PIPE", "SKF_WGRAD_OCC", "SKF_WG_ABLATE_SPLIT", "SKF_WG_ABLATE_LOAD", "SKF_WSX_ABLATE_LOAD", "SKF_WSX_ABLATE_STORE",
    "SKF_WSX_ABLATE_MFMA", "SKF_WSX_FENCES", "SKF_WSX_EARLY3", "SKF_WS_STAMPS", "SKF_FFN_ABLATE", "SKF_FFN_STAMPS", "SKF_PH8_ABLATE",
    "SKF_SPLIT_NO_DOT2", "SKF_ATTN_BWD_WAVES", "SKF_ATTN_BWD_TRP", "SKF_LN_FWD_GRID", "SKF_LN_BWD_GRID", "SKF_LN_UR", "SKF_LN_BWD_THREADS",
    "SKF_LN_BWD_UR", "SKF_DEC_UNROLL", "SKF_STAMP", "SKF_STAMP3", "SKF_FSTAMP", "FFN_STAMP",
)


# the translation units of the step orchestrator (skf_model_internal.h is what they share)
_MODEL_UNITS = ("skf_model", "skf_model_prof", "skf_model_layout", "skf_model_sched", "skf_model_fwd", "skf_model_bwd", "skf_model_decode",
                "skf_model_bf16")


def test_train_step_schedule_has_no_knobs():
    """The train step's stream / event schedule, the Dense / LayerNorm routing and the kernels' dispatch are fixed: the A/B knobs
    that once switched them are gone, and neither the library's sources and public header, the integration guide, the knob table of
    tools/ nor a tool (a script that still sets a dead variable or passes a dead -D) names a retired one.  The names are matched as
    whole words, also straight behind `-D`: no live identifier is one of them (SKF_ATTN_TWO_PASS, SKF_EXTRA_HIPCC_FLAGS, the
    SKF_MODEL_* flags and SKF_PREC_* stay)."""
    import glob
    csrc = os.path.join(ROOT, "sketchformer_amd", "csrc")
    units = sorted(os.path.basename(p) for p in glob.glob(os.path.join(csrc, "skf_model*")))
    for stem in _MODEL_UNITS:      # (a rename must not empty the loop below)
        assert any(u.startswith(stem + ".") for u in units), (stem, units)
    assert "skf_model_internal.h" in units
    for name in units:
        assert "skf_knob(" not in open(os.path.join(csrc, name)).read(), name
    pattern = re.compile(r"(?:\b|(?<=-D))(%s)\b" % "|".join(_RETIRED_KNOBS))
    assert pattern.search("hipcc -DSKF_MEASURE=1") and pattern.search("SKF_WS_XCD=0") and not pattern.search("SKF_ATTN_TWO_PASS SKF_EXTRA_HIPCC_FLAGS")
    docs = [os.path.join(ROOT, "INTEGRATION.md"), os.path.join(ROOT, "tools", "README.md"), os.path.join(ROOT, "include", "skf.h")]
    tools = [p for p in glob.glob(os.path.join(ROOT, "tools", "*")) if os.path.splitext(p)[1] in (".py", ".sh")]
    assert len(tools) > 40, tools
    for path in glob.glob(os.path.join(csrc, "*")) + docs + tools:
        m = pattern.search(open(path, encoding="utf-8").read())
        assert m is None, "%s names the retired knob %s" % (path, m.group(1))


def test_library_sources_are_the_build_list():
    """Every .hip file of csrc/ is compiled and nothing is textually included as code: a forgotten unit fails here, not at dlopen."""
    from sketchformer_amd import build
    csrc = os.path.join(ROOT, "sketchformer_amd", "csrc")
    files = sorted(os.listdir(csrc))
    assert sorted(f for f in files if f.endswith(".hip")) == sorted(build.SOURCES)
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    assert not [f for f in files if f.endswith(".inc")]
    for f in files:
        text = open(os.path.join(csrc, f), encoding="utf-8").read()
        m = re.search(r'#\s*include\s*"[^"\n]*\.(hip|inc)"', text)
        assert m is None, "%s: %s" % (f, m.group(0))


def test_library_has_no_unresolved_symbol_of_its_own(lib):
    """A helper that one unit declares (skf_model_internal.h) and no unit defines links into a shared library all the same and only
    fails when first called.  The weak `w _ZTH...` entries are the optional initialisers of the extern thread_local variables
    (null by design: both are constant-initialised); every other undefined symbol that names skf_ is a missing definition."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(ROOT, "sketchformer_amd", "libskf.so")],
                         capture_output=True, text=True, check=True).stdout
    lines = [ln.split() for ln in out.splitlines() if "skf_" in ln]
    assert len(out.splitlines()) > 20
    missing = [ln for ln in lines if not (ln[0] == "w" and ln[1].startswith("_ZTH"))]
    assert missing == [], missing


def test_launch_attached_events_and_input_handover_have_one_owner():
    """The thread-local slot that carries an event to a launcher's last launch (skf_tls_tail) is named in skf_common.h - the attach
    protocol: scope, chain helper, SKF_LAUNCH_TAIL - and at its single definition, nowhere else; the open-coded forms of the protocol
    are gone; and the Python layer reads its clone knob once instead of flipping an attribute around every step."""
    import glob
    pkg = os.path.join(ROOT, "sketchformer_amd")
    sources = [p for p in glob.glob(os.path.join(pkg, "**", "*"), recursive=True)
               if os.path.splitext(p)[1] in (".py", ".hip", ".h", ".inc")]
    assert len(sources) > 40, sources
    slot_lines = []
    for path in sources:
        text = open(path, encoding="utf-8").read()
        for gone in ("skf_tls_stop_event", "ParkedEventGuard", "take_ready", "_clone_inputs"):
            assert gone not in text, "%s still names %s" % (path, gone)
        if os.path.basename(path) != "skf_common.h":
            slot_lines += [(os.path.basename(path), ln.strip()) for ln in text.splitlines() if re.search(r"\bskf_tls_tail\b", ln)]
    assert len(slot_lines) == 1 and slot_lines[0][0] == "skf_model.hip", slot_lines
    assert slot_lines[0][1].startswith("thread_local SkfTailSlot skf_tls_tail;"), slot_lines
    header = open(os.path.join(pkg, "csrc", "skf_common.h")).read()
    assert header.count("extern thread_local") == 1 and "extern thread_local SkfTailSlot skf_tls_tail;" in header
    assert re.search(r"struct SkfTailSlot \{[^}]*hipEvent_t event[^}]*bool attached[^}]*\}", header)      # the event AND an explicit flag
    assert open(os.path.join(pkg, "engine.py")).read().count("SKF_CLONE_INPUTS") == 1
    assert "`SKF_CLONE_INPUTS=1`" in open(os.path.join(ROOT, "tools", "README.md")).read()


def test_step_scheduler_and_per_call_state_have_one_owner_each():
    """The two-stream scheduler's state lives in SideSched (declared in skf_model_internal.h, defined in skf_model_sched.hip) and is
    named nowhere else; what is valid during one call only lives in StepCtx; struct SkfModel declares neither set of members; and
    each routing decision of the row-owner launches is stated once."""
    import glob
    csrc = os.path.join(ROOT, "sketchformer_amd", "csrc")
    strip = lambda text: re.sub(r"//[^\n]*", "", text)      # noqa: E731  (code only: comments may speak of anything)
    units = {os.path.basename(p): strip(open(p, encoding="utf-8").read()) for p in glob.glob(os.path.join(csrc, "skf_model*"))}
    assert len(units) == len(_MODEL_UNITS) + 1 and "skf_model_internal.h" in units, sorted(units)
    header = units["skf_model_internal.h"]
    # the owners exist, with their single reset points
    sched = re.search(r"struct SideSched \{.*?\n\};", header, re.S)
    ctx = re.search(r"struct StepCtx \{.*?\n\};", header, re.S)
    model = re.search(r"\nstruct SkfModel \{.*?\n\};", header, re.S)
    assert sched and ctx and model
    sched, ctx, model = sched.group(0), ctx.group(0), model.group(0)
    assert re.search(r"\bSideSched sched;", model) and re.search(r"\bStepCtx ctx;", model)
    assert len(re.findall(r"\bvoid begin_backward\(\)", sched)) == 1 and len(re.findall(r"\bvoid reset\(\)", ctx)) == 1
    assert re.search(r"\bbool lists_set\b", ctx) and re.search(r"\blive_blocks\(int rows, int granule\)", ctx)
    scheduler_names = ("pending_readers", "pending_writers", "wq_held", "side_waited", "side_seq", "next_event")
    call_names = ("live16", "live32", "live_rows", "lists_built", "masks_staged", "pre_ready", "masks_ready", "last_ready")
    for name in scheduler_names:
        word = re.compile(r"\b%s\b" % name)
        assert word.search(sched), name                       # declared by the owner ...
        assert not word.search(header.replace(sched, "")), name      # ... and nowhere else in the header
        users = sorted(u for u, text in units.items() if word.search(text))
        assert users == ["skf_model_internal.h", "skf_model_sched.hip"], (name, users)
        begin = re.search(r"void begin_backward\(\) \{[^}]*\}", sched).group(0)
        if name not in ("side_waited", "side_seq"):           # (the two counters only ever grow)
            assert name in begin or (name == "next_event" and "rewind_events()" in begin), (name, begin)
    for name in scheduler_names + call_names:
        assert not re.search(r"\b%s\b" % name, model), "struct SkfModel declares %s" % name
    assert "M->ctx.reset()" in units["skf_model.hip"] and sum(text.count("ctx.reset()") for text in units.values()) == 1
    # the live-row expression, the row-owner routing predicate and the chained-projection width list are stated once
    sources = glob.glob(os.path.join(csrc, "*"))
    assert len(sources) > 30
    for path in sources:
        assert "live_rows) ?" not in open(path, encoding="utf-8").read(), path
    bwd, fwd = units["skf_model_bwd.hip"], units["skf_model_fwd.hip"]
    # top-level functions of the backward unit (a body ends at the first `}` in column 0) that compare against ln_part_stride
    bodies = re.findall(r"^[A-Za-z][^\n;]*\b(\w+)\([^;{]*\) \{\n(.*?)^\}", bwd, re.S | re.M)
    assert len(bodies) >= 8 and {"ffn_ln_bwd", "ln_oproj_bwd", "run_backward"} <= {n for n, _ in bodies}, [n for n, _ in bodies]
    comparing = [n for n, body in bodies if re.search(r"[<>=!]=?\s*(M->plan|P)\.ln_part_stride|ln_part_stride\s*[<>=!]", body)]
    assert comparing == ["row_owner_takes_ln"] and bwd.count("ln_part_stride") == 1, comparing
    for caller in ("ffn_ln_bwd", "ln_oproj_bwd", "run_backward"):
        assert dict(bodies)[caller].count("row_owner_takes_ln(") == 1, caller
    assert "SKF_CHECK_ARG(!lead_a" in dict(bodies)["ln_oproj_bwd"] and "ln_oproj_bwd_takes_lead" not in bwd
    assert fwd.count("== 384") == 1 and fwd.count("chains(M, ") >= 3


def test_gemm_wsx_isa_has_no_crossed_select_packed_fp32():
    """Round 4 bisected the run-to-run wrong results of round 3's 'accumulate only' epilogue kind to a compiler-formed
    v_pk_add_f32 with crossed operand selects in gemm_wsx_kernel's exit block (skf_gemm_wsx.hip: launch_wsx).  The kind is gone; this
    keeps the dominant kernel family free of the instruction form (a new epilogue that lets the compiler pair adds again shows up
    here, on the CPU, before it shows up as a flaky gradient on the GPU)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("isa_pk_opsel", os.path.join(ROOT, "tools", "isa_pk_opsel.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    path, hits = mod.scan(os.path.join(ROOT, "sketchformer_amd", "csrc", "skf_gemm_wsx.hip"), [])
    assert hits is not None, "skf_gemm_wsx.hip did not compile"
    assert hits == {}, hits


def test_host_only_entry_points(lib):
    from sketchformer_amd import _lib, engine
    assert lib.skf_version() >= 100
    cfg = engine.make_config(batch=4, seq_len=24, d_model=64, num_heads=4, dff=128, num_layers=2, vocab_size=52,
                             n_classes=7, lowerdim=32)
    assert lib.skf_config_validate(C.byref(cfg)) == 0
    entries = engine.param_entries(cfg)
    n = lib.skf_model_param_floats(C.byref(cfg))
    assert n > 0 and lib.skf_model_workspace_bytes(C.byref(cfg)) > 0
    # layout is a partition: no overlap, inside the buffer
    import numpy as np
    used = np.zeros(n, dtype=np.int32)
    for e in entries:
        for r in range(e["rows"]):
            used[e["offset"] + r * e["row_stride"]: e["offset"] + r * e["row_stride"] + e["cols"]] += 1
    assert used.max() == 1


def test_layout_names_match_oracle(lib):
    import oracle
    from sketchformer_amd import engine
    ocfg = oracle.Config(num_layers=2, d_model=64, dff=128, num_heads=4, lowerdim=32, vocab_size=52, n_classes=7, seq_len=24)
    cfg = engine.make_config(batch=4, seq_len=24, d_model=64, num_heads=4, dff=128, num_layers=2, vocab_size=52,
                             n_classes=7, lowerdim=32)
    want = {n: s for n, s, _ in oracle.param_specs(ocfg)}
    got = {e["name"]: engine.logical_shape(e) for e in engine.param_entries(cfg)}
    assert got == want


@pytest.mark.parametrize("kw", [dict(do_classification=False), dict(do_reconstruction=False),
                                dict(lowerdim=0, do_classification=False), dict(do_reconstruction=False, attn_version=2, lowerdim=64)])
def test_structural_variant_layouts_match_oracle(lib, kw):
    """do_classification / do_reconstruction off, lowerdim=0 (models/sketchformer.py:76-108): the variable set shrinks."""
    import oracle
    from sketchformer_amd import engine
    base = dict(num_layers=2, d_model=64, dff=128, num_heads=4, lowerdim=32, vocab_size=52, n_classes=7, seq_len=24)
    base.update(kw)
    ocfg = oracle.Config(**base)
    cfg = engine.make_config(batch=4, **base)
    want = [(n, s) for n, s, _ in oracle.param_specs(ocfg)]
    got = [(e["name"], engine.logical_shape(e)) for e in engine.param_entries(cfg)]
    assert dict(got) == dict(want)
    assert [n for n, _ in got if "/mha" not in n] == [n for n, _ in want if "/mha" not in n]


@pytest.mark.parametrize("attn_version,cbuf", [(2, 0), (1, 2), (2, 1)])
def test_variant_layout_names_match_oracle(lib, attn_version, cbuf):
    """SelfAttnV2 (builders/layers/transformer.py:76-131: W (d,d), Dense(lowerdim) -> embedding width = lowerdim, which is
    also the cross-attention K/V input width) and class_buffer_layers (models/sketchformer.py:101-104)."""
    import oracle
    from sketchformer_amd import engine
    ocfg = oracle.Config(num_layers=2, d_model=64, dff=128, num_heads=4, lowerdim=128, vocab_size=52, n_classes=7, seq_len=24,
                         attn_version=attn_version, class_buffer_layers=cbuf)
    cfg = engine.make_config(batch=4, seq_len=24, d_model=64, num_heads=4, dff=128, num_layers=2, vocab_size=52,
                             n_classes=7, lowerdim=128, attn_version=attn_version, class_buffer_layers=cbuf)
    want = {n: s for n, s, _ in oracle.param_specs(ocfg)}
    got = {e["name"]: engine.logical_shape(e) for e in engine.param_entries(cfg)}
    assert got == want
    assert [e["name"] for e in engine.param_entries(cfg) if "/mha" not in e["name"]] == \
           [n for n, _, _ in oracle.param_specs(ocfg) if "/mha" not in n]          # same forward order


def test_unsupported_configs_fail_loudly(lib):
    from sketchformer_amd import engine
    cfg = engine.make_config(batch=4, lowerdim=0)                       # class head without a bottleneck: the reference fails too
    assert lib.skf_config_validate(C.byref(cfg)) == -1
    assert b"lowerdim" in lib.skf_last_error()
    assert lib.skf_config_validate(C.byref(engine.make_config(batch=4, lowerdim=0, do_classification=False))) == 0
    assert lib.skf_config_validate(C.byref(engine.make_config(batch=4, do_reconstruction=False))) == 0
    assert lib.skf_config_validate(C.byref(engine.make_config(batch=4, do_reconstruction=False, do_classification=False))) == -1
    # any d_model % num_heads == 0 like the reference (MFMA kernels for the BASELINE widths, skf_generic.hip for the others), within
    # d_model % 4 == 0, head size % 4 == 0, d_model <= 1024, head size <= 128
    assert lib.skf_config_validate(C.byref(engine.make_config(batch=4, d_model=96))) == 0         # 8 heads of 12
    assert lib.skf_config_validate(C.byref(engine.make_config(batch=4, d_model=80, num_heads=2))) == 0
    assert lib.skf_config_validate(C.byref(engine.make_config(batch=4, d_model=100, num_heads=8))) == -1      # not divisible by the heads
    assert lib.skf_config_validate(C.byref(engine.make_config(batch=4, d_model=72, num_heads=4))) == -2       # head size 18
    assert b"head size" in lib.skf_last_error()
    assert lib.skf_config_validate(C.byref(engine.make_config(batch=4, d_model=2048, num_heads=32))) == -2
    assert lib.skf_config_validate(C.byref(engine.make_config(batch=4, attn_version=3))) == -1
    assert lib.skf_config_validate(C.byref(engine.make_config(batch=4, attn_version=2, lowerdim=100))) == 0
    assert lib.skf_config_validate(C.byref(engine.make_config(batch=4, attn_version=2, lowerdim=102))) == -2
    assert lib.skf_config_validate(C.byref(engine.make_config(batch=4, attn_version=2, class_buffer_layers=2, optimizer="sgd"))) == 0
    with pytest.raises(ValueError):
        engine.make_config(batch=4, optimizer="rmsprop")
    assert lib.skf_config_validate(C.byref(engine.make_config(batch=4, continuous=True, vocab_size=None))) == 0
    with pytest.raises(TypeError):
        engine.make_config(batch=4, lr_scheduler="step-decay")


@pytest.mark.parametrize("d_model,num_heads,precision,longest", [
    (512, 8, None, 224),       # head size 64: the one-pass backward holds Q / dO of 224 rows (the forward would take 288 keys)
    (512, 8, 0, 224),
    (256, 8, None, 448),       # head size 32: two-pass backward up to 256, then the one-pass kernel up to 448 rows
    (256, 8, 0, 448),
    (128, 8, None, 512),       # head size 16 fits at the longest sequence the model takes
    (128, 8, 0, 512),
    (96, 8, None, 512),        # head size 12: the plain kernels of skf_generic.hip take 1024 positions
])
def test_fp32_sequence_limits_of_the_attention_launches_are_refused_at_validate(lib, d_model, num_heads, precision, longest):
    """skf_attention_fwd / skf_attention_bwd keep one head's operands in LDS and refuse what does not fit; skf_config_validate
    holds seq_len against the same size functions (hand arithmetic from fwd_smem / bwd_smem of skf_attention.hip: 160 KB hold
    288 key rows forward and 224 query rows backward at head size 64, 448 query rows backward at head size 32, 512 at 16), so
    such a model is refused when it is configured and not inside its first step.  The bf16 path streams its keys: unaffected."""
    from sketchformer_amd import engine
    mk = lambda L, **kw: engine.make_config(batch=4, seq_len=L, d_model=d_model, num_heads=num_heads, gemm_precision=precision, **kw)
    assert lib.skf_config_validate(C.byref(mk(longest))) == 0, lib.skf_last_error()
    assert lib.skf_config_validate(C.byref(mk(longest - 15))) == 0
    if longest < 512:
        dh = d_model // num_heads
        assert lib.skf_config_validate(C.byref(mk(longest + 1))) == -2
        msg = lib.skf_last_error().decode()
        assert "head size %d" % dh in msg and "%d query rows" % longest in msg and "%d keys" % (288 if dh == 64 else 512) in msg, msg
        assert lib.skf_config_validate(C.byref(mk(512))) == -2
    else:
        assert lib.skf_config_validate(C.byref(mk(513))) == -1          # the model's own limit
    if d_model == 512:
        assert lib.skf_config_validate(C.byref(mk(512, act_dtype="bf16", vocab_size=1004))) == 0, lib.skf_last_error()


def test_continuous_layout_names_match_oracle(lib):
    import oracle
    from sketchformer_amd import engine
    ocfg = oracle.Config(num_layers=6, d_model=256, dff=1024, num_heads=8, lowerdim=256, n_classes=345, seq_len=200, continuous=True)
    cfg = engine.make_config(batch=4, num_layers=6, d_model=256, dff=1024, continuous=True, vocab_size=None)
    want = {n: s for n, s, _ in oracle.param_specs(ocfg)}
    got = {e["name"]: engine.logical_shape(e) for e in engine.param_entries(cfg)}
    assert got == want
    assert sum(int(np.prod(s)) for s in want.values()) == 11218670        # P for cfg 3


def test_param_count_matches_survey(lib):
    """P = 2,316,117 for cfg 2 (C=345), 2,271,741 for cfg 1 (C=1)."""
    from sketchformer_amd import engine
    for C_, want in ((345, 2316117), (1, 2271741)):
        cfg = engine.make_config(batch=128, n_classes=C_)
        assert sum(e["rows"] * e["cols"] for e in engine.param_entries(cfg)) == want


def test_reduce_batch_add_checks_the_bias_gradient_contract_before_anything_else():
    """include/skf.h, SkfReduceDesc: the batched reduction has no scalar path, so a descriptor with a bias gradient needs a 16-byte
    aligned slab and M*N % 4 == 0.  The launch cannot check a device array; ReduceBatch::add is the one place every descriptor of
    the model passes on the host, and the refusal is its first statement (before the descriptor is stored or counted)."""
    text = open(os.path.join(ROOT, "sketchformer_amd", "csrc", "skf_model_sched.hip")).read()
    body = re.search(r"int ReduceBatch::add\(const SkfReduceDesc& d, int blocks\) \{(.*?)\n\}", text, flags=re.S).group(1)
    code = re.sub(r"//[^\n]*", "", body).strip()
    first = code.split(";")[0]
    assert first.startswith("SKF_CHECK_ARG("), first
    assert "!d.bias_grad ||" in first and "(uintptr_t)d.slab & 15" in first and "(size_t)d.M * d.N) & 3" in first, first
    # and no descriptor with a bias gradient is built around it: the only one that names a gradient is the weight-gradient
    # descriptor of skf_model_sched.hip, handed to add in the next statement; the tables built elsewhere carry nullptr
    csrc = os.path.join(ROOT, "sketchformer_amd", "csrc")
    named = []
    for f in sorted(f for f in os.listdir(csrc) if f.startswith("skf_model")):       # the units that build SkfReduceDesc tables
        for value in re.findall(r"\.bias_grad = ([^;]+);", open(os.path.join(csrc, f)).read()):
            if value.strip() != "nullptr":
                named.append(f)
    assert named == ["skf_model_sched.hip"], named
    assert re.search(r"d\.bias_grad = M->G\(w\.b\);[^\n]*\n[^\n]*\n\s*SKF_TRY\(M->red\.add\(d,", text)


def test_no_cpu_fallback():
    import torch
    from sketchformer_amd import engine, _lib
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.SkfError):
        engine.TrainEngine(engine.make_config(batch=4))
