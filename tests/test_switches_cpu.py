"""The host-side switch table (segmminterest_amd/switches.py): the only place of the package that reads SEGMM_* variables
(hipabi's SEGMM_LIB / SEGMM_GEMM apart), its defaults and parsing, what a store is constructed with, and the retired names.
The expected values are written out here; none is derived from the table under test."""
import ast
import glob
import os

import pytest

from helpers import ROOT
from segmminterest_amd import switches

# (environment name, owners, attribute, default value, {spelling: parsed value})
EXPECTED = [
    ("SEGMM_OVERLAP", "engine", "overlap", True, {"0": False, "1": True}),
    ("SEGMM_DEFER_WGRAD", "engine", "defer_wgrad", None, {"auto": None, "0": False, "1": True}),
    ("SEGMM_LN_SIDE", "engine", "ln_side", None, {"auto": None, "0": False, "1": True}),
    ("SEGMM_LAZY_HEAD_GRAD", "engine", "lazy_head_grad", True, {"0": False, "1": True}),
    ("SEGMM_HEAD_DOT", "engine", "head_dot", True, {"0": False, "1": True}),
    ("SEGMM_SIDE_PRIORITY", "engine trainer", "side_priority", 1, {"0": 0, "1": 1, "-1": -1}),
    ("SEGMM_ATTN_PLANES_ONLY", "engine", "attn_planes_only", 1, {"0": 0, "1": 1, "2": 2}),
    ("SEGMM_ATT_PL", "engine", "attn_pl", 1, {"0": 0, "1": 1, "2": 2}),
    ("SEGMM_EU_PLANES_ONLY", "engine", "eu_planes_only", True, {"0": False, "1": True}),
    ("SEGMM_INPUT_PLANES_ONLY", "engine", "input_planes_only", True, {"0": False, "1": True}),
    ("SEGMM_SCALING", "engine", "scaling", "delayed", {"delayed": "delayed", "exact": "exact", "always": "always"}),
    ("SEGMM_SCALE_TARGET", "engine", "scale_target", 7, {"7": 7, "12": 12}),
    ("SEGMM_LOSS_RELATIVE", "engine", "loss_relative", True, {"0": False, "1": True}),
    ("SEGMM_PLANES", "engine", "planes", True, {"0": False, "1": True}),
    ("SEGMM_WGRAD", "engine", "wgrad_planes", 3, {"x6": 3, "x3": 2}),
    ("SEGMM_GEMM_BN", "engine", "gemm_bn", "", {"": "", "128": "128", "256": "256"}),
    ("SEGMM_SPLIT_TARGET", "engine", "split_target", 1024, {"1024": 1024, "512": 512}),
    ("SEGMM_SPLIT_TARGET_P", "engine", "split_target_p", 256, {"256": 256, "128": 128}),
    ("SEGMM_SPLIT_TARGET_FEW", "engine", "split_target_few", 256, {"256": 256, "512": 512}),
    ("SEGMM_SPARSE_TABLES", "trainer", "sparse_tables", True, {"0": False, "1": True}),
    ("SEGMM_BUCKET_ADAMW", "trainer", "per_bucket_adamw", True, {"0": False, "1": True}),
    ("SEGMM_TABLE_TWO_PASS", "trainer", "table_two_pass", True, {"0": False, "1": True}),
    ("SEGMM_BEGIN_OVERLAP", "trainer", "begin_overlap", True, {"0": False, "1": True}),
    ("SEGMM_DP_BUCKET_MB", "trainer", "bucket_mb", 8.0, {"8": 8.0, "0.5": 0.5, "25": 25.0}),
    ("SEGMM_DP_FORCE", "comm", "force", False, {"0": False, "1": True}),
]
RETIRED = ["SEGMM_ATTN_FUSED", "SEGMM_ATTN_SPLIT", "SEGMM_ATTN_TWO_STREAMS", "SEGMM_FEW_TILES", "SEGMM_LN_POS", "SEGMM_TAIL_BALANCE",
           "SEGMM_HEAD_SIDE", "SEGMM_USR_SIDE", "SEGMM_FWD_SIDE"]


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in list(os.environ):
        if k.startswith("SEGMM_"):
            monkeypatch.delenv(k)


def _env_uses(path):
    """(line, name read or written) of every use of os.environ / os.getenv / os.putenv in a source file; the name is the first
    string literal of the enclosing call or subscript (None when there is none)."""
    tree = ast.parse(open(path).read())
    parents = {c: p for p in ast.walk(tree) for c in ast.iter_child_nodes(p)}
    uses = []
    for node in ast.walk(tree):
        hit = (isinstance(node, ast.Attribute) and node.attr in ("environ", "getenv", "putenv")) or \
              (isinstance(node, ast.Name) and node.id in ("environ", "getenv", "putenv"))
        if not hit:
            continue
        top = node
        while top in parents and not isinstance(top, (ast.Call, ast.Subscript)):
            top = parents[top]
        names = [n.value for n in ast.walk(top) if isinstance(n, ast.Constant) and isinstance(n.value, str)]
        uses.append((node.lineno, names[0] if names else None))
    return uses


def test_the_package_reads_the_environment_in_switches_only():
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "segmminterest_amd", "*.py"))):
        name = os.path.basename(path)
        if name != "switches.py":
            for _, var in _env_uses(path):
                found.setdefault(name, []).append(var)
    assert found == {"hipabi.py": ["SEGMM_LIB", "SEGMM_GEMM"], "my_evaluation.py": ["PYTHONHASHSEED"]}
    assert _env_uses(os.path.join(ROOT, "segmminterest_amd", "switches.py"))          # (the walk does see the reads that exist)


def test_defaults_and_parsing_of_every_row(monkeypatch):
    assert sorted(sw.env for sw in switches.TABLE) == sorted(e[0] for e in EXPECTED)
    by_env = {sw.env: sw for sw in switches.TABLE}
    for env, owners, attr, default, spellings in EXPECTED:
        sw = by_env[env]
        assert (sw.attr, sorted(sw.owners)) == (attr, sorted(owners.split())), env
        for owner in owners.split():
            got = switches.read(owner)[attr]
            assert got == default and type(got) is type(default), (env, owner, got)
            for text, value in spellings.items():
                monkeypatch.setenv(env, text)
                got = switches.read(owner)[attr]
                assert got == value and type(got) is type(value), (env, owner, text, got)
            monkeypatch.delenv(env)
    for owner in ("engine", "trainer", "comm"):
        assert sorted(switches.read(owner)) == sorted(e[2] for e in EXPECTED if owner in e[1].split())


def _store(monkeypatch, **env):
    from segmminterest_amd.trainer import default_args, init_model
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    margs = default_args(num_layers_enc=2, d_model=32, nhead=2, input_type={"user": "image", "photo": "image"}, exposure_prob=[1.0] * 8)
    return init_model(margs, input_dim=32, max_vid_len=8, max_usr_len=4)._store


def test_a_store_is_constructed_with_the_documented_values(monkeypatch):
    from segmminterest_amd import hipabi as H
    st = _store(monkeypatch)
    plane = H.GEMM_ENGINE == H.ENGINE_F16X3P
    want = dict(overlap=True, lazy_head_grad=True, head_dot=True, defer_wgrad=False, ln_side=False, defer_wgrad_forced=None,
                ln_side_forced=None, side_priority=1, attn_planes_only=1, attn_pl=1, eu_planes_only=True, input_planes_only=True,
                scaling="delayed", scale_target=7, loss_relative=True, wgrad_planes=3, gemm_bn="", split_target=1024,
                split_target_p=256, split_target_few=256, engine_p=plane,
                use_planes=H.GEMM_ENGINE in (H.ENGINE_BF16X6, H.ENGINE_F16X3))
    for k, v in want.items():
        got = getattr(st, k)
        assert got == v and type(got) is type(v), (k, got)
    assert st.defer_wgrad is False and st.ln_side is False and st.attn_pl == 1 and st.attn_planes_only == 1 and st.scale_target == 7
    for gone in ("ln_pos", "tail_balance", "head_side", "usr_side", "fwd_side", "attn_fused", "attn_split", "attn_two_streams",
                 "_defer_wgrad_env", "_ln_side_env"):
        assert not hasattr(st, gone), gone


def test_a_store_reads_the_environment_when_it_is_constructed(monkeypatch):
    st = _store(monkeypatch, SEGMM_DEFER_WGRAD="1", SEGMM_ATT_PL="0", SEGMM_LN_SIDE="0")
    assert st.defer_wgrad is True and st.defer_wgrad_forced is True and st.attn_pl == 0
    assert st.ln_side is False and st.ln_side_forced is False          # forced off: not left to the backward's S > 32 rule
    monkeypatch.delenv("SEGMM_DEFER_WGRAD")
    assert _store(monkeypatch).defer_wgrad is False                    # read again by the next construction


def test_dump_lists_every_row_once_and_retired_names_raise(monkeypatch):
    lines = switches.dump().split("\n")
    assert len(lines) == len(switches.TABLE) == len(EXPECTED)
    names = [ln.split("=", 1)[0] for ln in lines]
    assert len(set(names)) == len(names) and sorted(names) == sorted(e[0] for e in EXPECTED)
    for ln in lines:
        assert "  # " in ln and ln.split("  # ", 1)[1].strip(), ln          # NAME=value  # doc
    assert "SEGMM_SCALE_TARGET=7  # " in switches.dump()
    monkeypatch.setenv("SEGMM_SCALE_TARGET", "12")
    assert "SEGMM_SCALE_TARGET=12  # " in switches.dump()
    assert sorted(switches.RETIRED) == sorted(RETIRED) and not set(switches.RETIRED) & set(names)
    for name in RETIRED:
        monkeypatch.setenv(name, "0")
        for owner in ("engine", "trainer", "comm"):
            with pytest.raises(RuntimeError, match=name):
                switches.read(owner)
        monkeypatch.delenv(name)
    switches.read("engine")
