"""Parameter groups of FusedAdamW, the parts that need no GPU: group resolution and segments (pure functions of names, sizes and
offsets), the ``state_dict`` format against torch.optim.AdamW, and the three new entry points in the ABI tables."""
import fnmatch
import math

import pytest
import torch

from helpers import build_model, load_case

NEW = ("segmm_adamw_groups", "segmm_grad_norm_groups", "segmm_adamw_table_lrs")


@pytest.fixture(scope="module")
def model():
    cfg, _, _, _ = load_case("img_d32_N2")
    return build_model(cfg)


def _named(model):
    return list(model.named_parameters())


def _layout(model):
    """[(name, offset, numel)] the way ParamStore._build lays parameters out, without the store: model order, every parameter at
    the next multiple of 32 floats -- and n_live."""
    order, off = [], 0
    for n, p in model.named_parameters():
        off = (off + 31) & ~31
        order.append((n, off, p.numel()))
        off += p.numel()
    return order, (off + 7) & ~7


def test_entry_points_in_the_abi_tables():
    from segmminterest_amd import hipabi as H
    L = H.lib()
    assert H.ABI_VERSION == 30 and L.segmm_abi_version() == 30
    names = {L.segmm_cmd_op_name(i).decode() for i in range(L.segmm_cmd_op_count())}
    for n in NEW:
        assert n in H.SIGNATURES and hasattr(L, n), n
        assert n in names, n          # a recorded step can carry it
    assert H.PARAMS["segmm_adamw_groups"] == ("p", "g", "m", "v", "start", "n", "seg_end", "seg_lr_scale", "seg_weight_decay", "seg_frozen",
                                              "n_seg", "lr", "beta1", "beta2", "eps", "step", "coef", "stream")
    # nothing that existed changed its prototype
    assert len(H.SIGNATURES["segmm_adamw"]) == 12 and len(H.SIGNATURES["segmm_adamw_table"]) == 17
    assert len(H.SIGNATURES["segmm_adamw_table_scaled"]) == 17 and len(H.SIGNATURES["segmm_grad_norm"]) == 6


def test_new_entry_points_reject_bad_arguments():
    from segmminterest_amd import hipabi as H
    L = H.lib()
    p, g, m, v, e, s, w, f, c = (4096 * k for k in range(1, 10))          # never dereferenced: every call fails its argument check

    def err(rc):
        assert rc != 0
        return L.segmm_last_error().decode()

    hp = (1e-3, 0.9, 0.999, 1e-8)
    assert "pointer" in err(L.segmm_adamw_groups(p, None, m, v, 0, 8, e, s, w, f, 1, *hp, 1, None, None))
    assert "segment table" in err(L.segmm_adamw_groups(p, g, m, v, 0, 8, None, s, w, f, 1, *hp, 1, None, None))
    assert "segment table" in err(L.segmm_adamw_groups(p, g, m, v, 0, 8, e, s, w, f, 0, *hp, 1, None, None))
    assert "start=2" in err(L.segmm_adamw_groups(p, g, m, v, 2, 8, e, s, w, f, 1, *hp, 1, None, None))
    assert "step=0" in err(L.segmm_adamw_groups(p, g, m, v, 0, 8, e, s, w, f, 1, *hp, 0, None, None))
    assert "needs step == -1" in err(L.segmm_adamw_groups(p, g, m, v, 0, 8, e, s, w, f, 1, H.LIVE_LR, 0.9, 0.999, 1e-8, 3, None, None))
    sc, o2 = 8192 * 5, 8192 * 6
    assert "segment table" in err(L.segmm_grad_norm_groups(g, 8, e, None, 1, 1.0, sc, o2, None))
    assert "16-byte" in err(L.segmm_grad_norm_groups(g + 4, 8, e, f, 1, 1.0, sc, o2, None))
    assert "max_norm" in err(L.segmm_grad_norm_groups(g, 8, e, f, 1, 0.0, sc, o2, None))
    ids, flags = 4096 * 11, 4096 * 12
    tab = (10, 8, ids, 3, flags)
    for bad in (-0.5, math.inf, float("nan")):
        assert "lr_scale" in err(L.segmm_adamw_table_lrs(p, g, m, v, *tab, 1e-3, bad, 0.9, 0.999, 1e-8, 0.0, 1, 1, None, None)), bad
    assert "phase 1 only" in err(L.segmm_adamw_table_lrs(p, None, m, v, *tab, 1e-3, 0.1, 0.9, 0.999, 1e-8, 0.0, 1, 0, c, None))
    assert "needs g" in err(L.segmm_adamw_table_lrs(p, None, m, v, *tab, 1e-3, 0.1, 0.9, 0.999, 1e-8, 0.0, 1, 1, None, None))


def test_patterns_and_callables_select_the_expected_names(model):
    from segmminterest_amd.trainer import resolve_param_groups
    named = _named(model)
    names = [n for n, _ in named]
    pats = ["*.bias", "*ln_*.weight", "*_ln.weight", "*_pe.weight"]
    groups = resolve_param_groups(named, [
        {"params": pats, "weight_decay": 0.0},
        {"params": ["stage_mlp1.weight"], "lr_scale": 0.1},
        {"params": lambda n, p: n.startswith("backbone1.encoder.layers.1.") and p.dim() == 2, "frozen": True},
    ], 1e-2)
    assert len(groups) == 4
    want1 = [n for n in names if any(fnmatch.fnmatchcase(n, q) for q in pats)]
    assert groups[1]["names"] == want1 and len(want1) > 10
    assert (groups[1]["lr_scale"], groups[1]["weight_decay"], groups[1]["frozen"]) == (1.0, 0.0, False)
    assert groups[2]["names"] == ["stage_mlp1.weight"]
    assert groups[2]["lr_scale"] == float(torch.tensor(0.1, dtype=torch.float32)) and groups[2]["weight_decay"] == groups[0]["weight_decay"]
    want3 = [n for n, p in named if n.startswith("backbone1.encoder.layers.1.") and p.dim() == 2]
    assert groups[3]["names"] == want3 and groups[3]["frozen"] is True
    taken = set(want1) | {"stage_mlp1.weight"} | set(want3)
    assert groups[0]["names"] == [n for n in names if n not in taken]          # the default group: everything else, model order
    assert (groups[0]["lr_scale"], groups[0]["frozen"]) == (1.0, False)
    assert groups[0]["weight_decay"] == float(torch.tensor(1e-2, dtype=torch.float32))
    assert sorted(sum((G["names"] for G in groups), [])) == sorted(names)
    # no groups at all: one default group holding everything
    (only,) = resolve_param_groups(named, [], 1e-4)
    assert only["names"] == names


def test_bad_groups_are_refused_by_name(model):
    from segmminterest_amd.trainer import FusedAdamW, resolve_param_groups
    named = _named(model)
    with pytest.raises(ValueError, match=r"both select the parameter stage_mlp1\.bias"):
        resolve_param_groups(named, [{"params": ["*.bias"]}, {"params": ["stage_mlp1.*"]}], 0.0)
    with pytest.raises(ValueError, match=r"'\*\.no_such_thing' selects no parameter"):
        resolve_param_groups(named, [{"params": ["*.bias", "*.no_such_thing"]}], 0.0)
    with pytest.raises(ValueError, match="selects no parameter"):
        resolve_param_groups(named, [{"params": lambda n, p: False}], 0.0)
    for key in ("betas", "eps", "lr", "momentum"):
        with pytest.raises(ValueError, match="unknown key '%s'" % key):
            resolve_param_groups(named, [{"params": ["*.bias"], key: 0.5}], 0.0)
    for key in ("lr_scale", "weight_decay"):
        for bad in (-1.0, float("nan"), math.inf, "0.1", True, 1e39):
            with pytest.raises(ValueError, match=key):
                resolve_param_groups(named, [{"params": ["*.bias"], key: bad}], 0.0)
    with pytest.raises(ValueError, match="frozen"):
        resolve_param_groups(named, [{"params": ["*.bias"], "frozen": 1}], 0.0)
    with pytest.raises(ValueError, match="params"):
        resolve_param_groups(named, [{"lr_scale": 0.5}], 0.0)
    # the optimizer resolves at construction, before any device is needed
    with pytest.raises(ValueError, match=r"'nope\.\*' selects no parameter"):
        FusedAdamW(model, param_groups=[{"params": ["nope.*"]}])
    opt = FusedAdamW(model, weight_decay=1e-2, param_groups=[{"params": ["*.bias"], "weight_decay": 0.0, "lr_scale": 3}])
    assert opt.group_of("stage_mlp1.bias") == (3.0, 0.0, False)
    assert opt.group_of("stage_mlp1.weight") == (1.0, float(torch.tensor(1e-2, dtype=torch.float32)), False)
    assert FusedAdamW(model, weight_decay=0.5).group_of("stage_mlp1.weight") == (1.0, 0.5, False)
    with pytest.raises(KeyError, match="nope"):
        opt.group_of("nope")


def test_segments_merge_neighbours_and_end_on_multiples_of_4(model):
    from segmminterest_amd.trainer import group_segments, no_decay_groups, resolve_param_groups
    named = _named(model)
    order, n_live = _layout(model)
    groups = resolve_param_groups(named, no_decay_groups(model) + [{"params": ["stage_mlp1.weight"], "lr_scale": 0.1}], 1e-2)
    gi = {n: k for k, G in enumerate(groups) for n in G["names"]}

    def hyper(n):
        G = groups[gi[n]]
        return G["lr_scale"], G["weight_decay"], G["frozen"]

    segs = group_segments(order, n_live, hyper)
    ends = [s[0] for s in segs]
    assert ends == sorted(set(ends)) and ends[-1] == n_live
    assert all(e % 4 == 0 for e in ends[:-1])
    assert all(a[1:] != b[1:] for a, b in zip(segs, segs[1:]))          # maximal: neighbours differ
    # fewer segments than parameters: runs of biases / LayerNorm weights, and runs of matrices, have merged
    assert 2 < len(segs) < len(order)
    # every parameter lies, gap behind it included, in a segment with its own values
    starts = [0] + ends[:-1]
    for n, off, k in order:
        (s,) = [i for i, (a, b) in enumerate(zip(starts, ends)) if a <= off < b]
        assert segs[s][1:] == hyper(n) and off + k <= ends[s], n
    # one group: one segment over everything
    assert group_segments(order, n_live, lambda n: (1.0, 0.25, False)) == [(n_live, 1.0, 0.25, False)]
    # a parameter that starts off a multiple of 4 cannot begin a segment
    with pytest.raises(AssertionError, match="multiple of 4"):
        group_segments([("a", 0, 6), ("b", 6, 8)], 16, lambda n: (1.0, 0.0, n == "b"))
    # ... but may sit inside one
    assert group_segments([("a", 0, 6), ("b", 6, 8)], 16, lambda n: (2.0, 0.0, False)) == [(16, 2.0, 0.0, False)]


def test_no_decay_groups_selects_biases_layernorms_and_positional_tables(model):
    from segmminterest_amd.trainer import no_decay_groups
    for case in ("img_d32_N2", "id_d32_N2"):
        mdl = model if case == "img_d32_N2" else build_model(load_case(case)[0])
        (g,) = no_decay_groups(mdl)
        assert g["weight_decay"] == 0.0 and set(g) == {"params", "weight_decay"}
        mods = dict(mdl.named_modules())
        want = []
        for n, _ in mdl.named_parameters():
            owner, leaf = n.rsplit(".", 1)
            if leaf == "bias" or isinstance(mods[owner], torch.nn.LayerNorm) or owner.endswith("_pe"):
                want.append(n)
        assert sorted(g["params"]) == sorted(want)
        assert any(n.endswith("vid_pe.weight") for n in want) and any(n.endswith("_ln.weight") for n in want)
        assert not any(n.endswith("_proj.weight") or n == "stage_mlp1.weight" for n in g["params"])


class _Store:
    """What FusedAdamW.state_dict reads of a ParamStore, on the CPU: the layout of the live parameters."""

    def __init__(self, model, dead):
        order, self.n_live = _layout(model)
        self._params = dict(model.named_parameters())
        self.index = {n: (o, k) for n, o, k in order}
        self.live_names = [n for n, _, _ in order if n not in dead]
        self.flat = torch.zeros(self.n_live)

    def ensure(self):
        pass


def test_state_dict_loads_into_torch_adamw_with_the_same_index_groups(model):
    from segmminterest_amd.trainer import FusedAdamW, no_decay_groups
    frozen = [n for n, _ in model.named_parameters() if n.startswith("backbone1.encoder.layers.0.ff_vid.")]
    dead = {"backbone1.encoder.patch_merge.0.weight", "backbone1.encoder.patch_merge.0.bias"}
    pg = no_decay_groups(model)
    pg[0]["params"] = [n for n in pg[0]["params"] if n not in frozen]
    pg += [{"params": ["stage_mlp1.weight"], "lr_scale": 0.1, "weight_decay": 0.0}, {"params": frozen, "frozen": True}]
    opt = FusedAdamW(model, lr=1e-3, weight_decay=1e-2, param_groups=pg)
    model._store = st = _Store(model, dead)
    try:
        opt.m, opt.v = torch.rand(st.n_live), torch.rand(st.n_live)
        opt._flat_id, opt.step_count = st.flat.data_ptr(), 7
        opt._build_segments(st)
        sd = opt.state_dict()
    finally:
        del model._store
    names = [n for n, _ in model.named_parameters()]
    groups = sd["param_groups"]
    assert len(groups) == 4
    assert [g["segmm_lr_scale"] for g in groups] == [1.0, 1.0, float(torch.tensor(0.1, dtype=torch.float32)), 1.0]
    assert groups[0]["lr"] == 1e-3 and groups[0]["weight_decay"] == 1e-2 and groups[1]["weight_decay"] == 0.0
    assert groups[2]["lr"] == float(torch.tensor(1e-3, dtype=torch.float32) * torch.tensor(0.1, dtype=torch.float32))
    assert groups[3]["params"] == [] and [names[i] for i in groups[3]["segmm_frozen_params"]] == frozen
    listed = sorted(i for g in groups for i in g["params"])
    assert listed == [i for i, n in enumerate(names) if n not in frozen]          # dead parameters stay listed, as without groups
    assert set(sd["state"]) == {i for i, n in enumerate(names) if n not in frozen and n not in dead}
    # torch.optim.AdamW built with the same index groups accepts the dict, state and hyperparameters
    clones = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    topt = torch.optim.AdamW([{"params": [clones[i] for i in g["params"]]} for g in groups], lr=1.0)
    topt.load_state_dict(sd)
    for tg, g in zip(topt.param_groups, groups):
        assert tg["lr"] == g["lr"] and tg["weight_decay"] == g["weight_decay"] and tg["segmm_lr_scale"] == g["segmm_lr_scale"]
    i = names.index("stage_mlp1.weight")
    o, k = st.index["stage_mlp1.weight"]
    assert torch.equal(topt.state[clones[i]]["exp_avg"].reshape(-1), opt.m[o:o + k]) and float(topt.state[clones[i]]["step"]) == 7.0
    assert all(clones[names.index(n)] not in topt.state for n in frozen)
    # without groups the format is what it was: one entry, no extra key
    (g1,) = _plain(model, st).state_dict()["param_groups"]
    assert "segmm_lr_scale" not in g1 and g1["params"] == list(range(len(names)))


def _plain(model, st):
    from segmminterest_amd.trainer import FusedAdamW
    opt = FusedAdamW(model)

    class M:          # state_dict reads model._store and named_parameters only
        _store = st
        named_parameters = model.named_parameters
    opt.model = M
    opt.m, opt.v, opt._flat_id = torch.zeros(st.n_live), torch.zeros(st.n_live), st.flat.data_ptr()
    return opt


def test_load_state_dict_refuses_another_grouping_by_name(model):
    from segmminterest_amd.trainer import FusedAdamW, no_decay_groups
    st = _Store(model, set())

    def make(pg):
        opt = FusedAdamW(model, param_groups=pg)

        class M:
            _store = st
            named_parameters = model.named_parameters
            parameters = model.parameters
        opt.model = M
        opt.m, opt.v, opt._flat_id = torch.zeros(st.n_live), torch.zeros(st.n_live), st.flat.data_ptr()
        if opt.groups is not None:
            opt._build_segments(st)
        return opt

    sd = make(no_decay_groups(model)).state_dict()
    make(no_decay_groups(model)).load_state_dict(sd)          # the same grouping loads
    with pytest.raises(ValueError, match=r"load_state_dict: .*parameter backbone1\.\S+\.bias"):
        make([{"params": ["stage_mlp1.*"], "lr_scale": 0.5}]).load_state_dict(sd)
    with pytest.raises(ValueError, match=r"load_state_dict: .*parameter \S+"):
        make(None).load_state_dict(sd)          # a grouped checkpoint into an optimizer without groups
    with pytest.raises(ValueError, match=r"load_state_dict: .*parameter \S+"):
        make(no_decay_groups(model)).load_state_dict(make(None).state_dict())
    # the groups' values come back from the checkpoint
    src = make([{"params": ["stage_mlp1.*"], "lr_scale": 0.5, "weight_decay": 0.25}])
    dst = make([{"params": ["stage_mlp1.*"], "lr_scale": 2.0}])
    dst.load_state_dict(src.state_dict())
    assert dst.group_of("stage_mlp1.bias") == (0.5, 0.25, False) and dst.group_table() == src.group_table()
    # a one-group checkpoint loads into a plain optimizer as ever, and into param_groups=[]
    make(None).load_state_dict(make(None).state_dict())
    make([]).load_state_dict(make(None).state_dict())
