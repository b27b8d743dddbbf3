"""Argument checks of the fused launches (tt_launch's eight role sets) and of the positional exports
that share their argument builders, on a GPU-less host: every case is a plan or call that is valid
except for ONE defect, so it must come back as a status code and a message before any launch.
Host arrays (tables, features, cols, num_embeddings, block_sizes, owners, offsets, seg_off) are
real; device pointers are fake, suitably aligned addresses that are never dereferenced."""
import ctypes as C

import pytest

from two_tower_recommender_model_amd import _lib

EINVAL, ECAP = 1001, 1002
B, D, W, F = 256, 64, 2, 2
ML = 2 * B        # dedup max_lookups of the tower-side workspaces (two features of B lookups)
SLOTS = 64        # owner side: slots per source; W * SLOTS lookups
DD_CNT_MASK = (1 << 18) - 1

WGRAD, UPDATE, INSERT, RESOLVE = _lib.ROLE_WGRAD, _lib.ROLE_UPDATE, _lib.ROLE_INSERT, _lib.ROLE_RESOLVE
ADAGRAD, RCOUNT, RPLACE, GATHER = _lib.ROLE_ADAGRAD, _lib.ROLE_ROUTE_COUNT, _lib.ROLE_ROUTE_PLACE, _lib.ROLE_GATHER
TAIL = WGRAD | INSERT | ADAGRAD
WI = WGRAD | INSERT
UAR = UPDATE | ADAGRAD | RESOLVE
WA = WGRAD | ADAGRAD
UA = UPDATE | ADAGRAD
U = WGRAD | RCOUNT | ADAGRAD
U0 = RCOUNT | ADAGRAD
G = UPDATE | RPLACE | GATHER


def dev(i):
    """A fake device address: 1 MiB apart, so aligned for every check; never dereferenced."""
    return (i + 1) << 20


@pytest.fixture(scope="module")
def lib():
    from two_tower_recommender_model_amd.build import build

    build()
    return _lib.load()


class Env:
    """A valid set of arguments of every role (fresh arrays per instance; the instance keeps them alive)."""

    def __init__(self, lib):
        self.lib = lib
        self.shape = _lib.TowerShape(L=2, width=(C.c_int32 * 4)(128, 64, 0, 0), in_dim=(C.c_int32 * 2)(D, D),
                                     in_col=(C.c_int32 * 2)(0, D), flags=0)
        self.ws_bytes = lib.tt_tower_workspace_bytes(C.byref(self.shape), B)
        self.dd_bytes = lib.tt_dedup_workspace_bytes(ML)
        self.route_bytes = lib.tt_shard_route_workspace_bytes(F, B)
        assert self.ws_bytes > 0 and self.dd_bytes > 0 and self.route_bytes > 0
        self.tables = (_lib.TableMeta * 2)(_lib.TableMeta(0, 0, 1000, D, 0), _lib.TableMeta(1000 * D, 1000, 1000, D, 0))
        self.features = (_lib.FeatureMeta * 2)(_lib.FeatureMeta(0, 0, 0), _lib.FeatureMeta(1, D, 0))
        self.cols = (C.c_void_p * 2)(dev(20), dev(21))
        self.next_cols = (C.c_void_p * 2)(dev(22), dev(23))
        self.ne = (C.c_int64 * 2)(1000, 1000)
        self.block = (C.c_int64 * 2)(500, 0)   # feature 0 row-wise over 2 ranks, feature 1 table-wise
        self.owners = (C.c_int32 * 2)(0, 1)
        self.dd_tab = (C.c_int32 * 2)(0, 1)
        self.offsets = (C.c_int64 * 16)(*[4096 * q for q in range(16)])
        self.seg_off = (C.c_int64 * 2)(0, SLOTS // 2)
        self.wgrad = _lib.WgradRole(loss=dev(1), adam_step_state=dev(2), adam_lr=0.01, adam_beta1=0.9, adam_beta2=0.999)
        self.update = _lib.UpdateRole(params=dev(3), exp_avg=dev(4), exp_avg_sq=dev(5), eps=1e-8, beta1=0.9,
                                      beta2=0.999, weight_decay=0.0, grads_out=dev(6))
        self.update_rep = _lib.UpdateRole(params=dev(3), replicated=1, copies=W, base=dev(7), offsets=self.offsets,
                                          scale=0.5)
        self.insert = _lib.InsertRole(next_cols=self.next_cols, id_dtype=_lib.TT_I64, num_embeddings=self.ne,
                                      dedup_tables=self.dd_tab, next_dedup_ws=dev(8), dedup_ws_bytes=self.dd_bytes,
                                      dedup_max_lookups=ML)
        self.resolve = _lib.ResolveRole(dedup_ws=dev(8))
        self.route = _lib.RouteRole(F=F, id_dtype=_lib.TT_I64, cols=self.cols, num_embeddings=self.ne,
                                    block_sizes=self.block, owners=self.owners, W=W, segs=dev(10), send=dev(11),
                                    pos_in=dev(12), pos_out=dev(13), overflow=dev(14), route_ws=dev(15),
                                    route_ws_bytes=self.route_bytes)
        self.gather = _lib.GatherRole(weights=dev(16), tables=self.tables, T=2, recv=dev(17), block_i64=F + SLOTS,
                                      counts_i64=0, seg_off=self.seg_off, slots=SLOTS, rows_out=dev(18),
                                      out_stride=SLOTS, bad=dev(19), dedup_ws=dev(9), dedup_ws_bytes=self.dd_bytes,
                                      dedup_max_lookups=ML)
        self.wait = _lib.PeerWait(W=W, sys=0, flag=(C.c_void_p * 16)(dev(30), dev(31)), flags=dev(32), epoch=dev(33),
                                  err=dev(34), timeout_ticks=1000)
        self.direct = _lib.PeerDirect(W=W, first_row=(C.c_int64 * 16)(0, SLOTS), row0=(C.c_void_p * 16)(dev(35), dev(36)))

    def adagrad(self, multi_only):
        return _lib.AdagradRole(tables=self.tables, T=2, F=F, features=self.features, B=B, grad=dev(24), ldg=2 * D,
                                weights=dev(25), state=dev(26), lr=0.05, eps=1e-8, dedup_ws=dev(9),
                                dedup_ws_bytes=self.dd_bytes, dedup_max_lookups=ML, multi_only=multi_only)

    def plan(self, roles):
        """The valid plan of a role set (never launched: every case breaks it first)."""
        p = _lib.LaunchPlan(roles=roles, shape=C.pointer(self.shape), B=B, workspace=dev(0), ws_bytes=self.ws_bytes)
        if roles & WGRAD:
            p.wgrad = self.wgrad
        if roles & UPDATE:
            p.update = self.update_rep if roles == G else self.update
        if roles & INSERT:
            p.insert = self.insert
            if roles == TAIL:  # the ring tail's insert takes both sizes from the ADAGRAD role
                p.insert.dedup_ws_bytes = p.insert.dedup_max_lookups = 0
        if roles & RESOLVE:
            p.resolve = self.resolve
        if roles & ADAGRAD:
            p.adagrad = self.adagrad(1 if roles in (TAIL, UAR) else 0)
        if roles & (RCOUNT | RPLACE):
            p.route = self.route
        if roles & GATHER:
            p.gather = self.gather
        return p


def set_(path, value):
    """A defect: plan.<path> = value."""
    def f(e, p):
        obj = p
        *head, last = path.split(".")
        for h in head:
            obj = getattr(obj, h)
        setattr(obj, last, value)
    return f


def add_(path, delta):
    """A defect: plan.<path> += delta (a misaligned pointer, a size one byte short)."""
    def f(e, p):
        obj = p
        *head, last = path.split(".")
        for h in head:
            obj = getattr(obj, h)
        setattr(obj, last, getattr(obj, last) + delta)
    return f


def arr_(name, i, value):
    """A defect in a host array of the Env (the plan points at it)."""
    def f(e, p):
        getattr(e, name)[i] = value
    return f


def feat_off_(e, p):
    e.features[1].out_offset = D + 2


def wait_(e, p):
    p.wait = C.pointer(e.wait)


def wait_null_flags_(e, p):
    e.wait.flags = None
    p.wait = C.pointer(e.wait)


def direct_(**kw):
    def f(e, p):
        for k, v in kw.items():
            if k == "first_row1":
                e.direct.first_row[1] = v
            else:
                setattr(e.direct, k, v)
        p.gather.direct = C.pointer(e.direct)
    return f


# ---- the defects of each argument builder: (id, defect, status, identifying part of the message) ----
TOWER_WS = [  # the towers' workspace (every role set with WGRAD or UPDATE)
    ("tower_ws_short", add_("ws_bytes", -1), ECAP, "tower: workspace too small"),
    ("tower_ws_null", set_("workspace", None), ECAP, "tower: workspace too small"),
]
ADAGRAD_DEFECTS = [  # dedup_update_args
    ("adagrad_null_grad", set_("adagrad.grad", None), EINVAL, "dedup_rowwise_adagrad: null pointer"),
    ("adagrad_ws_misaligned", add_("adagrad.dedup_ws", 8), EINVAL, "dedup_rowwise_adagrad: workspace not 64-B aligned"),
    ("adagrad_ldg", set_("adagrad.ldg", 2 * D + 2), EINVAL, "ldg % 4 == 0"),
    ("adagrad_out_offset", feat_off_, EINVAL, "out_offset % 4 != 0"),
    ("adagrad_grad_misaligned", add_("adagrad.grad", 4), EINVAL, "16-B aligned"),
]
ADAGRAD_WS = [  # its workspace checks where no other role reads the same sizes first
    ("adagrad_ws_short", add_("adagrad.dedup_ws_bytes", -1), ECAP, "dedup_rowwise_adagrad: workspace too small"),
    ("adagrad_ws_null", set_("adagrad.dedup_ws", None), ECAP, "dedup_rowwise_adagrad: workspace too small"),
    ("adagrad_max_lookups_0", set_("adagrad.dedup_max_lookups", 0), EINVAL, "dedup_rowwise_adagrad: max_lookups out of range"),
    ("adagrad_max_lookups_huge", set_("adagrad.dedup_max_lookups", DD_CNT_MASK), EINVAL, "max_lookups out of range"),
    ("adagrad_max_lookups_below_FB", set_("adagrad.dedup_max_lookups", F * B - 1), ECAP, "F*B > max_lookups"),
]
ROUTE_DEFECTS = [  # the route builder, as reached from the fused launches (prefix "route")
    ("route_null_send", set_("route.send", None), EINVAL, "route: null pointer"),
    ("route_null_segs", set_("route.segs", None), EINVAL, "route: null pointer"),
    ("route_ws_short", add_("route.route_ws_bytes", -1), ECAP, "route: workspace too small"),
    ("route_owner_ge_W", arr_("owners", 1, W), EINVAL, "route: bad sharding of a feature"),
    ("route_blocks_exceed_W", arr_("block", 0, 100), EINVAL, "route: row blocks exceed the rank count"),
    ("route_null_col", arr_("cols", 0, None), EINVAL, "route: bad column"),
    ("route_id_dtype", set_("route.id_dtype", _lib.TT_F32), EINVAL, "route: ids must be int32/int64"),
    ("route_W_17", set_("route.W", 17), EINVAL, "route: "),
]
INSERT_COMMON = [
    ("insert_null_ws", set_("insert.next_dedup_ws", None), EINVAL, "null pointer"),
    ("insert_null_cols", set_("insert.next_cols", None), EINVAL, "null pointer"),
    ("insert_null_col", arr_("next_cols", 1, None), EINVAL, "tower insert: bad column / table"),
    ("insert_bad_table", arr_("dd_tab", 1, 64), EINVAL, "tower insert: bad column / table"),
    ("insert_id_dtype", set_("insert.id_dtype", _lib.TT_F32), EINVAL, "ids must be int32/int64"),
    ("insert_ws_misaligned", add_("insert.next_dedup_ws", 8), ECAP, "dedup workspace too small / misaligned"),
    ("wgrad_null_adam_state", set_("wgrad.adam_step_state", None), EINVAL, "null pointer"),
]
GATHER_DEFECTS = [  # gather_segs_args and launch G's direct stores
    ("gather_null_recv", set_("gather.recv", None), EINVAL, "shard_gather_segs: null pointer"),
    ("gather_rows_misaligned", add_("gather.rows_out", 4), EINVAL, "shard_gather_segs: D % 4 == 0 and aligned buffers"),
    ("gather_out_stride", set_("gather.out_stride", SLOTS - 1), EINVAL, "out_stride < slots"),
    ("gather_dd_ws_short", add_("gather.dedup_ws_bytes", -1), ECAP, "shard_gather_segs: dedup workspace too small / misaligned"),
    ("gather_dd_ws_misaligned", add_("gather.dedup_ws", 8), ECAP, "shard_gather_segs: dedup workspace too small / misaligned"),
    ("gather_dd_max_lookups_below_n", set_("gather.dedup_max_lookups", W * SLOTS - 1), ECAP, "shard_gather_segs: dedup workspace"),
    ("gather_dd_max_lookups_huge", set_("gather.dedup_max_lookups", DD_CNT_MASK), ECAP, "shard_gather_segs: dedup workspace"),
]
UPDATE_ADAM = [  # t3_args, Adam form
    ("update_null_params", set_("update.params", None), EINVAL, "tower: null pointer"),
    ("update_null_exp_avg", set_("update.exp_avg", None), EINVAL, "tower: null pointer"),
    ("update_replicated", set_("update.replicated", 1), EINVAL, "update.replicated = 0"),
]

LAUNCH_CASES = {
    TAIL: TOWER_WS + ADAGRAD_DEFECTS + INSERT_COMMON + [
        # the ring tail's insert takes its sizes from the ADAGRAD role and checks them first
        ("tail_ws_short", add_("adagrad.dedup_ws_bytes", -1), ECAP, "tower_tail: dedup workspace too small / misaligned"),
        ("tail_max_lookups_below_2B", set_("adagrad.dedup_max_lookups", 2 * B - 1), ECAP, "tower_tail: dedup workspace"),
        ("tail_max_lookups_0", set_("adagrad.dedup_max_lookups", 0), ECAP, "tower_tail: dedup workspace"),
        ("tail_max_lookups_huge", set_("adagrad.dedup_max_lookups", DD_CNT_MASK), ECAP, "tower_tail: dedup workspace"),
        ("tail_insert_bytes_differ", set_("insert.dedup_ws_bytes", 256), EINVAL, "two dedup workspaces have one size"),
        ("tail_insert_max_lookups_differ", set_("insert.dedup_max_lookups", ML + 1), EINVAL, "two dedup workspaces have one size"),
        ("tail_adagrad_ws_null", set_("adagrad.dedup_ws", None), ECAP, "dedup_rowwise_adagrad: workspace too small"),
        ("tail_multi_only_0", set_("adagrad.multi_only", 0), EINVAL, "multi_only"),
        ("tail_adagrad_B", set_("adagrad.B", B // 2), EINVAL, "adagrad.B"),
        ("tail_wait", wait_, EINVAL, "only launch U"),
    ],
    WI: TOWER_WS + INSERT_COMMON + [
        ("wi_ws_short", add_("insert.dedup_ws_bytes", -1), ECAP, "tower_wgrad_pre_insert: dedup workspace too small / misaligned"),
        ("wi_max_lookups_below_2B", set_("insert.dedup_max_lookups", 2 * B - 1), ECAP, "tower_wgrad_pre_insert: dedup workspace"),
        ("wi_max_lookups_0", set_("insert.dedup_max_lookups", 0), ECAP, "tower_wgrad_pre_insert: dedup workspace"),
        ("wi_max_lookups_huge", set_("insert.dedup_max_lookups", DD_CNT_MASK), ECAP, "tower_wgrad_pre_insert: dedup workspace"),
        ("wi_wait", wait_, EINVAL, "only launch U"),
    ],
    UAR: TOWER_WS + ADAGRAD_DEFECTS + ADAGRAD_WS + UPDATE_ADAM + [
        ("resolve_null", set_("resolve.dedup_ws", None), EINVAL, "tower_update_resolve: next dedup workspace null / misaligned"),
        ("resolve_misaligned", add_("resolve.dedup_ws", 8), EINVAL, "tower_update_resolve: next dedup workspace null / misaligned"),
        ("uar_multi_only_0", set_("adagrad.multi_only", 0), EINVAL, "multi_only"),
    ],
    WA: TOWER_WS + ADAGRAD_DEFECTS + ADAGRAD_WS + [
        ("wa_multi_only_1", set_("adagrad.multi_only", 1), EINVAL, "multi_only"),
        ("wa_wait", wait_, EINVAL, "only launch U"),
    ],
    UA: TOWER_WS + ADAGRAD_DEFECTS + ADAGRAD_WS + UPDATE_ADAM + [
        ("ua_multi_only_1", set_("adagrad.multi_only", 1), EINVAL, "multi_only"),
    ],
    U: TOWER_WS + ROUTE_DEFECTS + ADAGRAD_DEFECTS + ADAGRAD_WS + [
        ("u_null_adam_state", set_("wgrad.adam_step_state", None), EINVAL, "tower_wgrad_route_rowwise: null Adam step state"),
        ("u_wait_null_flags", wait_null_flags_, EINVAL, "tower_wgrad_route_rowwise: wait.W"),
        ("u_multi_only_1", set_("adagrad.multi_only", 1), EINVAL, "multi_only"),
    ],
    U0: ROUTE_DEFECTS + ADAGRAD_DEFECTS + ADAGRAD_WS + [
        ("u0_wait_null_flags", wait_null_flags_, EINVAL, "shard_route_count_rowwise_adagrad: wait.W"),
        ("u0_B_0", set_("B", 0), EINVAL, "route: "),
        ("u0_multi_only_1", set_("adagrad.multi_only", 1), EINVAL, "multi_only"),
    ],
    G: TOWER_WS + ROUTE_DEFECTS + GATHER_DEFECTS + [
        ("g_copies_0", set_("update.copies", 0), EINVAL, "tower_grads_replicated: bad output"),
        ("g_copies_17", set_("update.copies", 17), EINVAL, "tower_grads_replicated: bad output"),
        ("g_null_base", set_("update.base", None), EINVAL, "tower_grads_replicated: bad output"),
        ("g_null_params", set_("update.params", None), EINVAL, "tower_grads_replicated: bad output"),
        ("g_not_replicated", set_("update.replicated", 0), EINVAL, "update.replicated = 1"),
        ("g_direct_W", direct_(W=1), EINVAL, "tower_grads_place_gather: direct.W must be the route's W"),
        ("g_direct_first_row", direct_(first_row1=SLOTS - 1), EINVAL, "direct.first_row[s] must be s * out_stride"),
        ("g_direct_null_row0", direct_(row0=(C.c_void_p * 16)(dev(35), None)), EINVAL, "tower_grads_place_gather: direct.row0[d] is null"),
        ("g_wait", wait_, EINVAL, "only launch U"),
    ],
}
ROLE_NAMES = {TAIL: "tail", WI: "wgrad_insert", UAR: "update_adagrad_resolve", WA: "wgrad_adagrad",
              UA: "update_adagrad", U: "launch_u", U0: "launch_u_no_t2", G: "launch_g"}


def _launch_params():
    for roles, cases in LAUNCH_CASES.items():
        for cid, defect, code, msg in cases:
            yield pytest.param(roles, defect, code, msg, id=f"{ROLE_NAMES[roles]}-{cid}")


@pytest.mark.parametrize("roles,defect,code,msg", list(_launch_params()))
def test_launch_one_defect(lib, roles, defect, code, msg):
    e = Env(lib)
    p = e.plan(roles)
    defect(e, p)
    rc = lib.tt_launch(C.byref(p), None)
    got = lib.tt_last_error_string().decode()
    assert rc == code, (rc, got)
    assert msg in got, got


# ---- the positional exports on the shared builders ---------------------------------------------------
class Call:
    """The valid positional arguments of an export, by name; a case replaces one."""

    def __init__(self, fn, **kw):
        self.fn, self.kw = fn, kw

    def __call__(self, lib, **over):
        args = dict(self.kw)
        for k, v in over.items():
            assert k in args, k
            args[k] = v(args[k]) if callable(v) else v
        rc = getattr(lib, self.fn)(*args.values())
        return rc, lib.tt_last_error_string().decode()


def calls(e):
    sh = C.byref(e.shape)
    return {
        "tt_dedup_rowwise_adagrad": Call(
            "tt_dedup_rowwise_adagrad", tables=e.tables, T=2, features=e.features, F=F, B=B, grad=dev(24), ldg=2 * D,
            weights=dev(25), state=dev(26), lr=0.05, eps=1e-8, ws=dev(9), ws_bytes=e.dd_bytes, max_lookups=ML, stream=None),
        "tt_shard_route_segs": Call(
            "tt_shard_route_segs", F=F, B=B, cols=e.cols, id_dtype=_lib.TT_I64, ne=e.ne, block=e.block, owners=e.owners,
            W=W, segs=dev(10), send=dev(11), pos_in=dev(12), pos_out=dev(13), overflow=dev(14), ws=dev(15),
            ws_bytes=e.route_bytes, stream=None),
        "tt_shard_route_cols": Call(
            "tt_shard_route_cols", F=F, B=B, cols=e.cols, id_dtype=_lib.TT_I64, ne=e.ne, block=e.block, owners=e.owners,
            W=W, cap=B, send=dev(11), pos=dev(12), overflow=dev(14), ws=dev(15), ws_bytes=e.route_bytes, stream=None),
        "tt_shard_gather_segs_bf16": Call(
            "tt_shard_gather_segs_bf16", weights=dev(16), tables=e.tables, T=2, F=F, W=W, recv=dev(17),
            block_i64=F + SLOTS, counts_i64=0, seg_off=e.seg_off, slots=SLOTS, rows_out=dev(18), out_stride=SLOTS,
            bad=dev(19), dd_ws=dev(9), dd_bytes=e.dd_bytes, dd_max=ML, stream=None),
        "tt_tower_wgrad_pre": Call(
            "tt_tower_wgrad_pre", shape=sh, B=B, loss=dev(1), ws=dev(0), ws_bytes=e.ws_bytes, adam_state=dev(2), lr=0.01,
            beta1=0.9, beta2=0.999, dd_ws=dev(9), dd_bytes=e.dd_bytes, dd_max=ML, stream=None),
        "tt_tower_wgrad": Call("tt_tower_wgrad", shape=sh, B=B, loss=dev(1), ws=dev(0), ws_bytes=e.ws_bytes, stream=None),
        "tt_tower_update_pre": Call(
            "tt_tower_update_pre", shape=sh, B=B, params=dev(3), exp_avg=dev(4), exp_avg_sq=dev(5), eps=1e-8, beta1=0.9,
            beta2=0.999, wd=0.0, grads_out=dev(6), ws=dev(0), ws_bytes=e.ws_bytes, stream=None),
        "tt_tower_update": Call(
            "tt_tower_update", shape=sh, B=B, params=dev(3), exp_avg=dev(4), exp_avg_sq=dev(5), lr=0.01, beta1=0.9,
            beta2=0.999, eps=1e-8, wd=0.0, step_state=dev(2), do_adam=1, grads_out=dev(6), ws=dev(0),
            ws_bytes=e.ws_bytes, stream=None),
        "tt_tower_grads_replicated": Call(
            "tt_tower_grads_replicated", shape=sh, B=B, params=dev(3), base=dev(7), copies=W, offsets=e.offsets,
            scale=0.5, ws=dev(0), ws_bytes=e.ws_bytes, stream=None),
        "tt_tower_adam_pre_grads_sum": Call(
            "tt_tower_adam_pre_grads_sum", shape=sh, B=B, params=dev(3), grads=dev(7), nsrc=W, src_stride=1 << 20,
            exp_avg=dev(4), exp_avg_sq=dev(5), eps=1e-8, beta1=0.9, beta2=0.999, wd=0.0, ws=dev(0), ws_bytes=e.ws_bytes,
            wait=None, stream=None),
        "tt_tower_adam_grads": Call(
            "tt_tower_adam_grads", shape=sh, B=B, params=dev(3), grads=dev(7), exp_avg=dev(4), exp_avg_sq=dev(5), lr=0.01,
            beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, step_state=dev(2), ws=dev(0), ws_bytes=e.ws_bytes, stream=None),
    }


def _neg_offsets(e):
    e.offsets[1] = -4


def _bad_wait(e):
    e.wait.W = W + 1
    e.wait.flag[W] = dev(37)
    return C.pointer(e.wait)


short = lambda v: v - 1      # noqa: E731  (a size one byte short)
mis8 = lambda v: v + 8       # noqa: E731  (a pointer off its 64-B / 16-B alignment)

# (export, id, {argument: value or function of the valid value}, host-array defect, status, message part)
EXPORT_CASES = [
    ("tt_dedup_rowwise_adagrad", "null_grad", dict(grad=None), None, EINVAL, "dedup_rowwise_adagrad: null pointer"),
    ("tt_dedup_rowwise_adagrad", "ws_misaligned", dict(ws=mis8), None, EINVAL, "dedup_rowwise_adagrad: workspace not 64-B aligned"),
    ("tt_dedup_rowwise_adagrad", "ws_short", dict(ws_bytes=short), None, ECAP, "dedup_rowwise_adagrad: workspace too small"),
    ("tt_dedup_rowwise_adagrad", "ws_null", dict(ws=None), None, ECAP, "dedup_rowwise_adagrad: workspace too small"),
    ("tt_dedup_rowwise_adagrad", "max_lookups_0", dict(max_lookups=0), None, EINVAL, "max_lookups out of range"),
    ("tt_dedup_rowwise_adagrad", "max_lookups_below_FB", dict(max_lookups=F * B - 1), None, ECAP, "F*B > max_lookups"),
    ("tt_dedup_rowwise_adagrad", "ldg", dict(ldg=2 * D + 2), None, EINVAL, "ldg % 4 == 0"),
    ("tt_dedup_rowwise_adagrad", "out_offset", {}, lambda e: feat_off_(e, None), EINVAL, "out_offset % 4 != 0"),
    ("tt_dedup_rowwise_adagrad", "T_0", dict(T=0), None, EINVAL, "table count"),
]
for fn, pre in (("tt_shard_route_segs", "shard_route_segs"), ("tt_shard_route_cols", "shard_route")):
    EXPORT_CASES += [
        (fn, "null_send", dict(send=None), None, EINVAL, pre + ": null pointer"),
        (fn, "ws_short", dict(ws_bytes=short), None, ECAP, pre + ": workspace too small"),
        (fn, "ws_null", dict(ws=None), None, ECAP, pre + ": workspace too small"),
        (fn, "owner_ge_W", {}, lambda e: arr_("owners", 1, W)(e, None), EINVAL, pre + ": bad sharding of a feature"),
        (fn, "blocks_exceed_W", {}, lambda e: arr_("block", 0, 100)(e, None), EINVAL, pre + ": row blocks exceed the rank count"),
        (fn, "null_col", {}, lambda e: arr_("cols", 0, None)(e, None), EINVAL, pre + ": bad column"),
        (fn, "id_dtype", dict(id_dtype=_lib.TT_F32), None, EINVAL, pre + ": ids must be int32/int64"),
        (fn, "F_0", dict(F=0), None, EINVAL, pre + ": "),
        (fn, "W_17", dict(W=17), None, EINVAL, pre + ": "),
        (fn, "B_negative", dict(B=-1), None, EINVAL, pre + ": "),
    ]
EXPORT_CASES += [
    ("tt_shard_route_segs", "null_segs", dict(segs=None), None, EINVAL, "shard_route_segs: null pointer"),
    ("tt_shard_route_cols", "cap_0", dict(cap=0), None, EINVAL, "shard_route: "),
    ("tt_shard_gather_segs_bf16", "null_recv", dict(recv=None), None, EINVAL, "shard_gather_segs: null pointer"),
    ("tt_shard_gather_segs_bf16", "rows_misaligned", dict(rows_out=lambda v: v + 4), None, EINVAL, "aligned buffers"),
    ("tt_shard_gather_segs_bf16", "dd_ws_short", dict(dd_bytes=short), None, ECAP, "shard_gather_segs: dedup workspace too small / misaligned"),
    ("tt_shard_gather_segs_bf16", "dd_ws_misaligned", dict(dd_ws=mis8), None, ECAP, "shard_gather_segs: dedup workspace too small / misaligned"),
    ("tt_shard_gather_segs_bf16", "dd_max_below_n", dict(dd_max=W * SLOTS - 1), None, ECAP, "shard_gather_segs: dedup workspace"),
    ("tt_shard_gather_segs_bf16", "dd_max_huge", dict(dd_max=DD_CNT_MASK), None, ECAP, "shard_gather_segs: dedup workspace"),
    ("tt_shard_gather_segs_bf16", "seg_off_descending", {}, lambda e: arr_("seg_off", 1, -1)(e, None), EINVAL, "segment offsets must ascend"),
    ("tt_tower_wgrad_pre", "null_adam_state", dict(adam_state=None), None, EINVAL, "tower_wgrad_pre: null Adam step state"),
    ("tt_tower_wgrad_pre", "ws_short", dict(ws_bytes=short), None, ECAP, "tower: workspace too small"),
    ("tt_tower_wgrad_pre", "dd_ws_short", dict(dd_bytes=short), None, ECAP, "tower_wgrad_pre: dedup workspace too small / misaligned"),
    ("tt_tower_wgrad_pre", "dd_ws_misaligned", dict(dd_ws=mis8), None, ECAP, "tower_wgrad_pre: dedup workspace too small / misaligned"),
    ("tt_tower_wgrad_pre", "dd_max_0", dict(dd_max=0), None, ECAP, "tower_wgrad_pre: dedup workspace"),
    ("tt_tower_wgrad_pre", "dd_max_huge", dict(dd_max=DD_CNT_MASK), None, ECAP, "tower_wgrad_pre: dedup workspace"),
    ("tt_tower_wgrad", "ws_short", dict(ws_bytes=short), None, ECAP, "tower: workspace too small"),
    ("tt_tower_wgrad", "B_odd", dict(B=B + 4), None, EINVAL, "tower: B must be"),
    ("tt_tower_update_pre", "null_params", dict(params=None), None, EINVAL, "tower: null pointer"),
    ("tt_tower_update_pre", "null_exp_avg_sq", dict(exp_avg_sq=None), None, EINVAL, "tower: null pointer"),
    ("tt_tower_update_pre", "ws_short", dict(ws_bytes=short), None, ECAP, "tower: workspace too small"),
    ("tt_tower_update", "null_step_state", dict(step_state=None), None, EINVAL, "tower: null pointer"),
    ("tt_tower_update", "ws_null", dict(ws=None), None, ECAP, "tower: workspace too small"),
    ("tt_tower_grads_replicated", "copies_0", dict(copies=0), None, EINVAL, "tower_grads_replicated: bad output"),
    ("tt_tower_grads_replicated", "copies_17", dict(copies=17), None, EINVAL, "tower_grads_replicated: bad output"),
    ("tt_tower_grads_replicated", "null_base", dict(base=None), None, EINVAL, "tower_grads_replicated: bad output"),
    ("tt_tower_grads_replicated", "negative_offset", {}, _neg_offsets, EINVAL, "tower_grads_replicated: negative offset"),
    ("tt_tower_grads_replicated", "null_params", dict(params=None), None, EINVAL, "tower: null pointer"),
    ("tt_tower_grads_replicated", "ws_short", dict(ws_bytes=short), None, ECAP, "tower: workspace too small"),
    ("tt_tower_adam_pre_grads_sum", "null_grads", dict(grads=None), None, EINVAL, "tower_adam_pre_grads_sum: bad gradient"),
    ("tt_tower_adam_pre_grads_sum", "nsrc_0", dict(nsrc=0), None, EINVAL, "tower_adam_pre_grads_sum: bad gradient"),
    ("tt_tower_adam_pre_grads_sum", "src_stride_short", dict(src_stride=64), None, EINVAL, "tower_adam_pre_grads_sum: bad gradient"),
    ("tt_tower_adam_pre_grads_sum", "wait_W_not_nsrc", dict(wait=_bad_wait), None, EINVAL, "wait.W must be nsrc"),
    ("tt_tower_adam_pre_grads_sum", "null_exp_avg", dict(exp_avg=None), None, EINVAL, "tower: null pointer"),
    ("tt_tower_adam_pre_grads_sum", "ws_short", dict(ws_bytes=short), None, ECAP, "tower: workspace too small"),
    ("tt_tower_adam_grads", "null_grads", dict(grads=None), None, EINVAL, "tower_adam_grads: null gradient"),
    ("tt_tower_adam_grads", "null_step_state", dict(step_state=None), None, EINVAL, "tower: null pointer"),
    ("tt_tower_adam_grads", "ws_short", dict(ws_bytes=short), None, ECAP, "tower: workspace too small"),
]


@pytest.mark.parametrize("fn,over,host,code,msg", [pytest.param(fn, over, host, code, msg, id=f"{fn}-{cid}")
                                                   for fn, cid, over, host, code, msg in EXPORT_CASES])
def test_export_one_defect(lib, fn, over, host, code, msg):
    e = Env(lib)
    if host is not None:
        host(e)
    over = {k: (v(e) if v is _bad_wait else v) for k, v in over.items()}
    rc, got = calls(e)[fn](lib, **over)
    assert rc == code, (rc, got)
    assert msg in got, got


# ---- the dedup-workspace check: each call site's status for each defect ---------------------------------
def _dd_sites(e):
    """Every call site of the dedup-workspace check as (call, workspace / bytes / max_lookups argument
    names, minimum lookup count). The fused launches' sites are covered by test_launch_one_defect."""
    sh = C.byref(e.shape)
    two = lambda a, b: (C.c_void_p * 2)(a, b)  # noqa: E731
    e.keep = [two(dev(40), dev(41)), two(dev(42), dev(43))]
    return {
        "tt_tower_fwd_bwd_gather": (Call(
            "tt_tower_fwd_bwd_gather", shape=sh, B=B, cols=e.cols, id_dtype=_lib.TT_I64, ne=e.ne, rows=e.keep[0],
            pooled_out=None, ldp=2 * D, gpooled=dev(24), params=dev(3), labels=dev(27), label_dtype=_lib.TT_I32,
            grad_scale=1.0, logits=dev(28), dd_tab=e.dd_tab, dd_ws=dev(9), dd_bytes=e.dd_bytes, dd_max=ML, ws=dev(0),
            ws_bytes=e.ws_bytes, stream=None), 2 * B),
        "tt_tower_fwd_bwd_gather_update": (Call(
            "tt_tower_fwd_bwd_gather_update", shape=sh, B=B, cols=e.cols, id_dtype=_lib.TT_I64, ne=e.ne, rows=e.keep[0],
            state=e.keep[1], pooled_out=None, ldp=2 * D, gpooled=dev(24), params=dev(3), labels=dev(27),
            label_dtype=_lib.TT_I32, grad_scale=1.0, logits=dev(28), lr=0.05, eps=1e-8, dd_ws=dev(9),
            dd_bytes=e.dd_bytes, dd_max=ML, next_cols=None, ws=dev(0), ws_bytes=e.ws_bytes, stream=None), 2 * B),
        "tt_tower_wgrad_pre": (calls(e)["tt_tower_wgrad_pre"], 1),
        "tt_shard_gather_rows": (Call(
            "tt_shard_gather_rows", weights=dev(16), tables=e.tables, T=2, F=F, W=W, cap=SLOTS, recv=dev(17),
            rows_out=dev(18), bad=dev(19), dd_ws=dev(9), dd_bytes=e.dd_bytes, dd_max=ML, stream=None), W * F * SLOTS),
        "tt_shard_gather_segs_bf16": (calls(e)["tt_shard_gather_segs_bf16"], W * SLOTS),
    }


ONE_CODE_SITES = ["tt_tower_fwd_bwd_gather", "tt_tower_fwd_bwd_gather_update", "tt_tower_wgrad_pre",
                  "tt_shard_gather_rows", "tt_shard_gather_segs_bf16"]


@pytest.mark.parametrize("site", ONE_CODE_SITES)
@pytest.mark.parametrize("defect", ["short", "misaligned", "below_min", "huge"])
def test_dedup_ws_check_capacity_sites(lib, site, defect):
    """These call sites answer TT_ECAPACITY for every defect of the dedup workspace."""
    e = Env(lib)
    call, lo = _dd_sites(e)[site]
    over = {"short": dict(dd_bytes=short), "misaligned": dict(dd_ws=mis8), "below_min": dict(dd_max=lo - 1),
            "huge": dict(dd_max=DD_CNT_MASK)}[defect]
    rc, got = call(lib, **over)
    assert rc == ECAP, (rc, got)
    assert "dedup workspace too small / misaligned" in got, got


def _strict_sites(e):
    return {
        "tt_dedup_workspace_init": (Call("tt_dedup_workspace_init", ws=dev(9), ws_bytes=e.dd_bytes, max_lookups=ML,
                                         stream=None), "dedup_workspace_init"),
        "tt_dedup_resolve": (Call("tt_dedup_resolve", ws=dev(9), ws_bytes=e.dd_bytes, max_lookups=ML, stream=None),
                             "dedup_resolve"),
        "tt_dedup_insert_cols": (Call(
            "tt_dedup_insert_cols", tables=e.tables, T=2, features=e.features, F=F, B=B, cols=e.cols,
            id_dtype=_lib.TT_I64, ne=e.ne, ws=dev(9), ws_bytes=e.dd_bytes, max_lookups=ML, stream=None), "dedup_insert_cols"),
        "tt_dedup_insert_segments": (Call(
            "tt_dedup_insert_segments", keys=dev(17), counts=dev(18), nseg=W * F, cap=SLOTS, ws=dev(9),
            ws_bytes=e.dd_bytes, max_lookups=ML, stream=None), "dedup_insert_segments"),
        "tt_dedup_rowwise_adagrad": (calls(e)["tt_dedup_rowwise_adagrad"], "dedup_rowwise_adagrad"),
    }


@pytest.mark.parametrize("site", ["tt_dedup_workspace_init", "tt_dedup_resolve", "tt_dedup_insert_cols",
                                  "tt_dedup_insert_segments", "tt_dedup_rowwise_adagrad"])
@pytest.mark.parametrize("defect,code,msg", [("short", ECAP, "workspace too small"),
                                             ("null", ECAP, "workspace too small"),
                                             ("misaligned", EINVAL, "workspace not 64-B aligned"),
                                             ("huge", EINVAL, "max_lookups out of range")])
def test_dedup_ws_check_strict_sites(lib, site, defect, code, msg):
    """The dedup exports tell an out-of-range max_lookups and a misaligned workspace (TT_EINVAL)
    from a workspace that is too small (TT_ECAPACITY)."""
    e = Env(lib)
    call, pre = _strict_sites(e)[site]
    over = {"short": dict(ws_bytes=short), "null": dict(ws=None), "misaligned": dict(ws=mis8),
            "huge": dict(max_lookups=DD_CNT_MASK)}[defect]
    rc, got = call(lib, **over)
    assert rc == code, (rc, got)
    assert f"{pre}: {msg}" in got, got
