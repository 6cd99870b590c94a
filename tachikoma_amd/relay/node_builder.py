"""Builds a DeviceModule's native node list (tk_node) from its exec groups, one lowering per op.

``LOWERINGS`` maps a plan op name to its lowering ``(builder, node, op)``, ``GROUP_LOWERINGS`` a
fused group kind to ``(builder, node, group)``.  A lowering fills ``node`` (kind, attrs, ext) and
may replace ``builder.ins``; the driver loop (``NodeBuilder.build``) then writes the node's tensor
lists and emits it.  A lowering that emits its own nodes (layout convs, composites) leaves
``node.kind`` unset.  What the construction shares -- the node list, the shadows and which of them
are up to date, the shadow reads / writes waiting for the next node -- is the builder's state; the
buffers, kept objects and records stay on the module (``builder.m``)."""
from __future__ import annotations

import ctypes
from typing import Callable, Dict, List

import numpy as np

from .. import _lib
from .build_module import ExecGroup, PlanOp
from .qnn import legalize as _legalize
from .qnn import op as _qnn

KINDS = _lib.NODE_KINDS
TO_NCHW = (0, 3, 1, 2)
TO_NHWC = (0, 2, 3, 1)
LOWERINGS: Dict[str, Callable] = {}
GROUP_LOWERINGS: Dict[str, Callable] = {}


def lowers(*names: str, table: Dict[str, Callable] = LOWERINGS):
    def register(fn):
        for name in names:
            table[name] = fn
        return fn
    return register


def lowering_for(op_name: str) -> Callable:
    if op_name not in LOWERINGS:
        raise _lib.TachikomaError(f"no device lowering for {op_name}")
    return LOWERINGS[op_name]


# ---------------------------------------------------------------- fillers without device state
def transpose_attrs(perm):
    ta = _lib.tk_transpose_attrs()
    ta.ndim = len(perm)
    ta.perm[:len(perm)] = list(perm)
    return ta


def fill_rq_tensor(r, mode, multiplier, shift, input_zero_point, output_zero_point, axis=-1) -> None:
    """The scalar fields of a tk_requantize_attrs (all of them for a per-tensor requantize)."""
    r.mode, r.axis, r.multiplier, r.shift = mode, axis, multiplier, shift
    r.input_zero_point, r.output_zero_point = input_zero_point, output_zero_point


def conv_attrs(ca, a, consts, b: "NodeBuilder" = None) -> None:
    """tk_conv2d_attrs, tk_conv2d_transpose_attrs or tk_dense_attrs from an op's attrs: the geometry
    fields the struct has, the zero points (a float nn.conv2d has none) and, uploaded through the
    builder ``b``, per-channel kernel zero points."""
    for field in ("strides", "padding", "dilation", "output_padding"):
        if hasattr(ca, field):
            getattr(ca, field)[:] = list(a[field])
    if hasattr(ca, "groups"):
        ca.groups = a["groups"]
    ca.input_zero_point = a.get("input_zero_point", 0)
    ca.kernel_zero_point = a.get("kernel_zero_point", 0)
    if "kernel_zero_points" in consts:
        ca.kernel_zero_points = b.ptr(consts["kernel_zero_points"], np.int32)


def fill_qnn_add(qa, a) -> None:
    """tk_qnn_add_attrs from a lowered qnn.add (per-tensor RequantizeOrUpcast per side)."""
    for side in ("lhs", "rhs"):
        fill_rq_tensor(getattr(qa, side), a[f"{side}_mode"], a[f"{side}_multiplier"], a[f"{side}_shift"],
                       a[f"{side}_zero_point"], a["output_zero_point"])
    qa.output_zero_point, qa.lhs_upcast, qa.rhs_upcast = a["output_zero_point"], a["lhs_upcast"], a["rhs_upcast"]


class NodeBuilder:
    def __init__(self, m):
        self.m, self.lib = m, m.lib
        self.stream = _lib.stream_handle()
        self.nodes: List[_lib.tk_node] = []
        self.ins: List[_lib.TensorRef] = []   # of the node being built; a lowering may replace them
        self.outs: List[_lib.TensorRef] = []
        heads = [g.ops[0] for g in m.groups]
        # tensors read by MFMA convs need a shadow
        conv_ops = [op for op in heads if op.op in ("qnn.conv2d", "tachikoma.qnn.conv2d")]
        self.mfma = {op.name: self.is_mfma_conv(op) for op in conv_ops}
        # 8-bit max pools read their input's shadow too (16 channels per load) and write
        # their own output's shadow when an MFMA conv reads it
        pool_ops = [op for op in heads if op.op == "nn.max_pool2d" and op.out.dtype in ("int8", "uint8") and
                    len(op.out.shape) == 4]
        self.pool_names = {op.name for op in pool_ops}
        self.shadow_bufs: Dict[str, object] = {}
        for name in [self.conv_io(op)[0] for op in conv_ops if self.mfma[op.name]] + [op.inputs[0] for op in pool_ops]:
            if name not in self.shadow_bufs:
                self.shadow_bufs[name] = m._scratch(self.lib.tk_conv2d_shadow_bytes(m._ref(name).ptr), zero=True)
        self.shadow_ready = set()
        for name, buf in self.shadow_bufs.items():
            m.shadow_sources[f"shadow:{name}"] = (m._ref(name), buf)
        self.consts = {t.name for t in m.plan.params}
        # what the node being built reads / writes beside its plan inputs and records: the shadow
        # it reads (ensure_shadow) and the one its epilogue writes (shadow_out); taken by its emit
        self.pending_reads: List[str] = []
        self.pending_writes: List[str] = []

    def build(self) -> List[_lib.tk_node]:
        m = self.m
        for g in m.groups:
            head, n = g.ops[0], _lib.tk_node()
            self.outs = [m._ref(o.name) for o in g.ops]
            if g.kind in GROUP_LOWERINGS:
                GROUP_LOWERINGS[g.kind](self, n, g)
            else:
                lower = lowering_for(head.op)
                self.ins = [m._ref(x) for x in head.inputs]
                lower(self, n, head)
            if not n.kind:
                continue  # the lowering emitted its own nodes
            n.n_inputs = len(self.ins)
            for k, r in enumerate(self.ins):
                n.inputs[k] = r.ptr
            n.n_outputs = len(self.outs)
            for k, r in enumerate(self.outs):
                n.outputs[k] = r.ptr
            own = {o.name for o in g.ops}
            self.emit(n, g.kind, [o.name for o in g.ops], [x for o in g.ops for x in o.inputs if x not in own])
        return self.nodes

    # ------------------------------------------------------------ nodes and their records
    def emit(self, n, kind, records, reads=(), writes=(), shadows=None) -> None:
        m = self.m
        self.nodes.append(n)
        m.node_kinds.append(kind)
        m.node_native_kinds.append(int(n.kind))
        m.node_records.append(records)
        io = {"kind": kind, "records": list(records),
              "reads": [x for x in dict.fromkeys(reads) if x not in self.consts],
              "writes": list(dict.fromkeys(list(records) + list(writes))), "shadows": dict(shadows or {})}
        if kind != "shadow":
            io["reads"] += [x for x in self.pending_reads if x not in io["reads"]]
            for s in self.pending_writes:
                io["writes"].append(s)
                io["shadows"][s] = s[len("shadow:"):]
            self.pending_reads, self.pending_writes = [], []
        m.node_io.append(io)

    def shadow_node(self, ref, buf, name: str, source: str) -> None:
        """The node that fills the shadow ``name`` (``buf``) from ``source`` as the kernels see it (``ref``)."""
        sn = _lib.tk_node()
        sn.kind = KINDS["shadow"]
        sn.n_inputs, sn.n_outputs = 1, 0
        sn.inputs[0], sn.ext[0] = ref.ptr, buf.data_ptr()
        self.emit(sn, "shadow", [], [source], [name], {name: source})

    def ensure_shadow(self, name: str) -> None:
        """The node being built reads the shadow of ``name``: build it first unless an epilogue has."""
        self.pending_reads.append(f"shadow:{name}")
        if name not in self.shadow_ready:
            self.shadow_node(self.m._ref(name), self.shadow_bufs[name], f"shadow:{name}", name)
            self.shadow_ready.add(name)

    def shadow_out(self, n, name: str) -> None:
        """The epilogue of node ``n`` writes the shadow of its output ``name`` (the next MFMA conv reads it)."""
        n.ext[4] = self.shadow_bufs[name].data_ptr()
        self.shadow_ready.add(name)
        self.pending_writes.append(f"shadow:{name}")

    def transpose_node(self, src: str, dst: str, perm, records) -> None:
        t = _lib.tk_node()
        t.kind = KINDS["transpose"]
        t.attrs.transpose = transpose_attrs(perm)
        t.n_inputs, t.n_outputs = 1, 1
        t.inputs[0], t.outputs[0] = self.m._ref(src).ptr, self.m._ref(dst).ptr
        self.emit(t, "transpose", records, [src], [dst])

    def layout_in(self, op: PlanOp, L) -> None:
        """Where ``op``'s data is NHWC, the transpose into the buffer its NCHW kernel reads."""
        if L["x"] != op.inputs[0]:
            self.transpose_node(op.inputs[0], L["x"], TO_NCHW, [])

    def layout_out(self, c, op: PlanOp, L, x, w) -> None:
        """Emit the NCHW kernel ``c`` of ``op`` and, behind it, the transpose into the NHWC record."""
        c.n_inputs, c.n_outputs = 2, 1
        c.inputs[0], c.inputs[1] = x.ptr, w.ptr
        c.outputs[0] = self.m._ref(L["y"]).ptr
        self.emit(c, op.op, [] if L["y"] != op.name else [op.name], [L["x"]], [L["y"]])
        if L["y"] != op.name:
            self.transpose_node(L["y"], op.name, TO_NHWC, [op.name])

    # ------------------------------------------------------------ device memory
    def upload(self, array, dtype=None):
        """A node constant on the device, in ``dtype`` or its own (kept alive with the module)."""
        import torch
        t = torch.from_numpy(np.ascontiguousarray(array, dtype=dtype)).to(self.m.device)
        self.m._keep.append(t)
        return t

    def ptr(self, array, dtype=None) -> int:
        return self.upload(array, dtype).data_ptr()

    def sized(self, nbytes: int, what: str) -> int:
        """A byte count from the library; negative means it refused the shapes."""
        if nbytes < 0:
            _lib.check(_lib.TK_ERR_SHAPE, what)
        return nbytes

    def view_ref(self, name: str, shape) -> _lib.TensorRef:
        r = _lib.TensorRef.from_torch(self.m.buffers[name].view(*shape))
        self.m._keep.append(r)
        return r

    def dense_workspace(self, n) -> None:
        nbytes = self.lib.tk_qnn_dense_workspace_bytes(self.ins[0].ptr, self.ins[1].ptr)
        n.ext[0] = self.m._scratch(nbytes).data_ptr()

    # ------------------------------------------------------------ convolutions
    def conv_io(self, op: PlanOp):
        """(data buffer, weight buffer) the NCHW / OIHW conv kernels read for ``op``."""
        L = self.m.layout.get(op.name)
        return (L["x"], L["w"]) if L else (op.inputs[0], op.inputs[1])

    def conv_refs(self, op: PlanOp):
        """TensorRefs of the NCHW data and the OIHW grouped-conv weight for ``op``."""
        xn, wn = self.conv_io(op)
        L = self.m.layout.get(op.name)
        return self.m._ref(xn), (self.view_ref(wn, L["w_shape"]) if L else self.m._ref(wn))

    def is_mfma_conv(self, op: PlanOp) -> bool:
        ca = _lib.tk_conv2d_attrs()
        conv_attrs(ca, op.attrs, op.consts, self)
        x, w = self.conv_refs(op)
        ws = self.lib.tk_qnn_conv2d_workspace_bytes(x.ptr, w.ptr, ctypes.byref(ca))
        return self.sized(ws, f"{op.name} qnn.conv2d workspace") > 0

    def pack(self, param: str, what: str, weight: _lib.TensorRef, packed, sums) -> None:
        """Pack an MFMA conv weight (and its per-channel sums) now, and register the packing
        so that rewriting ``param`` (set_input / load_params) re-derives both."""
        def pack(s: int) -> None:
            _lib.check(self.lib.tk_conv2d_pack_weight(weight.ptr, 1, ctypes.c_void_p(packed.data_ptr()),
                                                      ctypes.c_void_p(sums.data_ptr()), ctypes.c_void_p(s)),
                       f"{what} pack weight")
        pack(self.stream)
        self.m._derived.setdefault(param, []).append(pack)

    def mfma_ext(self, n, op: PlanOp, x, w, shadow, ca) -> None:
        """ext slots of an MFMA conv (block) ``n``: shadow of the input, packed weight, weight sums
        (+ scratch: patch sums, split-K partial tiles)."""
        packed = self.m._scratch(self.lib.tk_conv2d_packed_weight_bytes(w.ptr, 1))
        sums = self.m._scratch(((w.shape[0] + 127) // 128 * 128) * 4)
        self.pack(op.inputs[1], op.name, w, packed, sums)
        n.ext[0], n.ext[1], n.ext[2] = shadow.data_ptr(), packed.data_ptr(), sums.data_ptr()
        block = int(n.kind == KINDS["conv_block"])
        nbytes = self.sized(self.lib.tk_conv2d_scratch_bytes(x.ptr, w.ptr, ctypes.byref(ca), block),
                            f"{op.name} conv scratch")
        if nbytes > 0:
            n.ext[3] = self.m._scratch(nbytes).data_ptr()

    def prep_conv(self, n, op: PlanOp, ca) -> None:
        """MFMA path of the conv (block) ``n`` reading ``self.ins``: its input's shadow and ext slots."""
        if self.mfma[op.name]:
            xname = self.conv_io(op)[0]
            self.ensure_shadow(xname)
            self.mfma_ext(n, op, self.ins[0], self.ins[1], self.shadow_bufs[xname], ca)

    def dense_as_conv(self, n, g: ExecGroup) -> bool:
        """A dense block [M, K] x [U, K]^T runs as a 1x1 conv block over [M, K, 1, 1]: the NCHW
        output [M, U, 1, 1] is the dense output's memory, requantize/bias stay on axis 1, and
        the conv path's weight packing happens once here instead of padding both operands on
        every run (the dense path's per-call pad_rows kernels).  Records are unchanged (same
        buffers).  Returns False (plain dense block) when the conv would not take MFMA."""
        head = g.ops[0]
        (m_, u), k = head.out.shape, self.m.plan.tensor(head.inputs[0]).shape[1]
        x4 = self.view_ref(head.inputs[0], (m_, k, 1, 1))
        w4 = self.view_ref(head.inputs[1], (u, k, 1, 1))
        ca = n.attrs.block.conv
        conv_attrs(ca, dict(head.attrs, strides=[1, 1], padding=[0, 0, 0, 0], dilation=[1, 1], groups=1),
                   head.consts, self)
        if self.lib.tk_qnn_conv2d_workspace_bytes(x4.ptr, w4.ptr, ctypes.byref(ca)) <= 0:
            n.attrs.block.conv = _lib.tk_conv2d_attrs()
            return False
        # shadow of the input (its producer is a flatten/copy node, which writes none)
        shadow = self.m._scratch(self.lib.tk_conv2d_shadow_bytes(x4.ptr), zero=True)
        sname = f"shadow:{head.name}:in"
        self.m.shadow_sources[sname] = (x4, shadow)
        self.shadow_node(x4, shadow, sname, head.inputs[0])
        self.pending_reads.append(sname)
        n.kind = KINDS["conv_block"]
        self.mfma_ext(n, head, x4, w4, shadow, ca)
        self.ins[0], self.ins[1] = x4, w4
        self.outs = [self.view_ref(o.name, tuple(o.out.shape) + (1, 1)) for o in g.ops]
        return True

    # ------------------------------------------------------------ requantize structs
    def rq_vectors(self, r, consts, multipliers: str, shifts: str, zero_points: str) -> None:
        """The per-channel vectors of a tk_requantize_attrs, where the plan has them."""
        if multipliers in consts:
            r.multipliers = self.ptr(consts[multipliers], np.int32)
            r.shifts = self.ptr(consts[shifts], np.int32)
        if zero_points in consts:
            r.input_zero_points = self.ptr(consts[zero_points], np.int32)

    def fill_rq(self, r, op: PlanOp) -> None:
        a = op.attrs
        fill_rq_tensor(r, a["mode"], a.get("multiplier", 0), a.get("shift", 0), a["input_zero_point"],
                       a["output_zero_point"], a["channel_axis"])
        self.rq_vectors(r, op.consts, "multipliers", "shifts", "input_zero_points")

    def fp_side(self, r, a, consts, prefix: str, axis: int, zp_key: str, zps_key: str, zp_out: int) -> None:
        """One tk_requantize_fp_attrs from a lowered plan's ``{prefix}fp_*`` attrs / consts."""
        r.rounding = _lib.TK_ROUND_UPWARD if a["rounding"] == "UPWARD" else _lib.TK_ROUND_TONEAREST
        r.bits, r.axis, r.scaled = a[f"{prefix}fp_bits"], axis, a[f"{prefix}fp_scaled"]
        r.multiplier = a[f"{prefix}fp_multiplier"]
        if f"{prefix}fp_multipliers" in consts:
            r.multipliers = self.ptr(consts[f"{prefix}fp_multipliers"], np.float64)
        r.input_zero_point, r.output_zero_point = a[zp_key], zp_out
        if zps_key in consts:
            r.input_zero_points = self.ptr(consts[zps_key], np.int32)

    def fill_binary(self, qb, op: PlanOp) -> None:
        """tk_qnn_binary_attrs / tk_qnn_binary_fp_attrs (float compute_dtype) from a lowered qnn.add /
        qnn.subtract / qnn.mul; a mul's operands keep no output zero point."""
        a = op.attrs
        fp = a.get("compute_dtype", "int64") != "int64"
        qb.op = _lib.TK_QB[op.op]
        for side in ("lhs", "rhs", "out"):
            if f"{side}_mode" not in a:
                continue
            r = getattr(qb, side)
            zp_out = 0 if op.op == "qnn.mul" and side != "out" else a["output_zero_point"]
            if not fp:
                fill_rq_tensor(r, a[f"{side}_mode"], a[f"{side}_multiplier"], a[f"{side}_shift"],
                               a[f"{side}_zero_point"], zp_out, a[f"{side}_axis"])
                self.rq_vectors(r, op.consts, f"{side}_multipliers", f"{side}_shifts", f"{side}_zero_points")
            elif f"{side}_fp_bits" in a:
                self.fp_side(r, a, op.consts, f"{side}_", a[f"{side}_axis"], f"{side}_zero_point",
                             f"{side}_zero_points", zp_out)
            else:  # an upcast side (add / subtract) or a mul operand: only its zero point(s) are read
                r.bits = 32 if a["compute_dtype"] == "float32" else 64
                r.axis, r.input_zero_point = a[f"{side}_axis"], a[f"{side}_zero_point"]
                if f"{side}_zero_points" in op.consts:
                    r.input_zero_points = self.ptr(op.consts[f"{side}_zero_points"], np.int32)
        qb.lhs_upcast, qb.rhs_upcast = a.get("lhs_upcast", 0), a.get("rhs_upcast", 0)
        qb.output_zero_point = a["output_zero_point"]


# ---------------------------------------------------------------- fused groups
@lowers("conv_block", "dense_block", table=GROUP_LOWERINGS)
def _block(b: NodeBuilder, n, g: ExecGroup) -> None:
    head, bias_op, rq_op = g.ops[:3]
    b.ins = [b.m._ref(head.inputs[0]), b.m._ref(head.inputs[1]), b.m._ref(bias_op.inputs[1])]
    ba = n.attrs.block
    b.fill_rq(ba.requantize, rq_op)
    add = g.add
    if add is not None:
        # residual join: the block's requantize output is one qnn.add operand
        ba.has_add = 1
        ba.block_is_rhs = int(add.inputs[1] == rq_op.name)
        b.ins.append(b.m._ref(add.inputs[0] if ba.block_is_rhs else add.inputs[1]))
        fill_qnn_add(ba.add, add.attrs)
    if g.last.op in ("clip", "nn.relu"):
        ba.has_clip, ba.clip_min, ba.clip_max = 1, g.last.attrs["lo"], g.last.attrs["hi"]
    if g.kind == "conv_block":
        n.kind = KINDS["conv_block"]
        conv_attrs(ba.conv, head.attrs, head.consts, b)
        b.prep_conv(n, head, ba.conv)
        if g.last.name in b.shadow_bufs:
            b.shadow_out(n, g.last.name)
    elif not b.dense_as_conv(n, g):
        n.kind = KINDS["dense_block"]
        conv_attrs(ba.dense, head.attrs, head.consts, b)
        b.dense_workspace(n)


@lowers("add_block", table=GROUP_LOWERINGS)
def _add_block(b: NodeBuilder, n, g: ExecGroup) -> None:
    head = g.ops[0]
    n.kind = KINDS["add_block"]
    b.ins = [b.m._ref(x) for x in head.inputs[:2]]
    ab = n.attrs.add_block
    fill_qnn_add(ab.add, head.attrs)
    if len(g.ops) == 2:
        ab.has_clip, ab.clip_min, ab.clip_max = 1, g.ops[1].attrs["lo"], g.ops[1].attrs["hi"]
    if g.last.name in b.shadow_bufs and len(head.out.shape) == 4:
        b.shadow_out(n, g.last.name)


@lowers("tachikoma.qnn.conv2d", "tachikoma.qnn.dense", table=GROUP_LOWERINGS)
def _composite(b: NodeBuilder, n, g: ExecGroup) -> None:
    """A tachikoma BYOC composite (relay/contrib/tachikoma.py) = two nodes: the contraction
    with zero zero points into an untraced int32 buffer, then tk_tachikoma_postops writing
    the composite's output (its one trace record, as the reference's composite function is
    one graph node)."""
    import torch
    op, m = g.ops[0], b.m
    acc = torch.empty(op.out.shape, dtype=torch.int32, device=m.device)
    acc_ref = _lib.TensorRef.from_torch(acc)
    m._keep += [acc, acc_ref]
    b.ins = [m._ref(op.inputs[0]), m._ref(op.inputs[1])]
    c = _lib.tk_node()
    if op.op == "tachikoma.qnn.conv2d":
        c.kind = KINDS["qnn.conv2d"]
        conv_attrs(c.attrs.conv2d, op.attrs, op.consts, b)
        b.prep_conv(c, op, c.attrs.conv2d)
    else:
        c.kind = KINDS["qnn.dense"]
        conv_attrs(c.attrs.dense, op.attrs, op.consts, b)
        b.dense_workspace(c)
    c.n_inputs, c.n_outputs = 2, 1
    c.inputs[0], c.inputs[1], c.outputs[0] = b.ins[0].ptr, b.ins[1].ptr, acc_ref.ptr
    acc_name = f"{op.name}:acc"
    b.emit(c, op.op + ":contraction", [], [op.inputs[0]], [acc_name])  # not a record
    p, a = _lib.tk_node(), op.attrs
    p.kind = KINDS["postops"]
    pa = p.attrs.postops
    pa.axis, pa.clip_lo, pa.clip_hi = 1, a["clip_lo"], a["clip_hi"]
    pa.act_scl, pa.sum_scl, pa.dst_zp = a["act_scl"], a["sum_scl"], a["dst_zp"]
    o_scl = b.upload(op.consts["postops_o_scl"])
    pa.bias, pa.o_scl = b.ptr(op.consts["postops_bias"]), o_scl.data_ptr()
    pa.n_scales = int(o_scl.numel())
    p.n_inputs, p.n_outputs = 1 + a["has_sum"], 1
    p.inputs[0], p.outputs[0] = acc_ref.ptr, m._ref(op.name).ptr
    if a["has_sum"]:
        p.inputs[1] = m._ref(op.inputs[2]).ptr
    b.emit(p, op.op, [op.name], [acc_name] + ([op.inputs[2]] if a["has_sum"] else []))


# ---------------------------------------------------------------- single ops
@lowers("qnn.conv2d")
def _qnn_conv2d(b: NodeBuilder, n, op: PlanOp) -> None:
    """NCHW / OIHW: one node.  NHWC data and/or another kernel layout: [transpose data -> NCHW], the
    NCHW / OIHW conv into an int32 NCHW buffer, [transpose -> the NHWC record]."""
    L = b.m.layout.get(op.name)
    c = _lib.tk_node() if L else n
    c.kind = KINDS["qnn.conv2d"]
    conv_attrs(c.attrs.conv2d, op.attrs, op.consts, b)
    if L:
        b.layout_in(op, L)
        b.ins = list(b.conv_refs(op))
    b.prep_conv(c, op, c.attrs.conv2d)
    if L:
        b.layout_out(c, op, L, b.ins[0], b.ins[1])


@lowers("qnn.conv2d_transpose")
def _qnn_conv2d_transpose(b: NodeBuilder, n, op: PlanOp) -> None:
    """[transpose NHWC data -> NCHW], the NCHW / IOHW kernel, [transpose -> the NHWC record]; a
    non-IOHW weight was transposed into "<op>:iohw_w" (re-derived on rewrite)."""
    L = b.m.layout.get(op.name, {"x": op.inputs[0], "w": op.inputs[1], "y": op.name})
    b.layout_in(op, L)
    c = _lib.tk_node()
    c.kind = KINDS["qnn.conv2d_transpose"]
    conv_attrs(c.attrs.conv2d_transpose, op.attrs, op.consts, b)
    b.layout_out(c, op, L, b.m._ref(L["x"]), b.m._ref(L["w"]))


@lowers("qnn.dense")
def _qnn_dense(b: NodeBuilder, n, op: PlanOp) -> None:
    n.kind = KINDS["qnn.dense"]
    conv_attrs(n.attrs.dense, op.attrs, op.consts, b)
    b.dense_workspace(n)


@lowers("qnn.batch_matmul")
def _qnn_batch_matmul(b: NodeBuilder, n, op: PlanOp) -> None:
    n.kind = KINDS[op.op]
    conv_attrs(n.attrs.dense, op.attrs, op.consts, b)
    ws = b.lib.tk_qnn_batch_matmul_workspace_bytes(b.ins[0].ptr, b.ins[1].ptr)
    if ws < 0:
        _lib.check(int(ws), f"{op.name} qnn.batch_matmul workspace")
    n.ext[0] = b.m._scratch(ws).data_ptr()


@lowers("qnn.requantize")
def _qnn_requantize(b: NodeBuilder, n, op: PlanOp) -> None:
    a = op.attrs
    if a.get("compute_dtype", "int64") != "int64":
        n.kind = KINDS["requantize_fp"]
        b.fp_side(n.attrs.requantize_fp, a, op.consts, "", a["channel_axis"], "input_zero_point", "input_zero_points",
                  a["output_zero_point"])
    else:
        n.kind = KINDS["qnn.requantize"]
        b.fill_rq(n.attrs.requantize, op)


@lowers("qnn.add", "qnn.subtract", "qnn.mul")
def _qnn_binary(b: NodeBuilder, n, op: PlanOp) -> None:
    a = op.attrs
    if a.get("compute_dtype", "int64") != "int64":
        n.kind = KINDS["qnn_binary_fp"]
        b.fill_binary(n.attrs.qnn_binary_fp, op)
    elif op.op == "qnn.add" and a.get("per_tensor"):
        n.kind = KINDS["qnn.add"]
        fill_qnn_add(n.attrs.qnn_add, a)
    else:
        n.kind = KINDS["qnn_binary"]
        b.fill_binary(n.attrs.qnn_binary, op)


@lowers("qnn.quantize", "qnn.dequantize")
def _qparams(b: NodeBuilder, n, op: PlanOp) -> None:
    n.kind = KINDS[op.op]
    qa, a = n.attrs.qparams, op.attrs
    qa.axis, qa.scale, qa.zero_point = a["axis"], a["scale"], a["zero_point"]
    if "scales" in op.consts:
        qa.scales = b.ptr(op.consts["scales"], np.float32)
    if "zero_points" in op.consts:
        qa.zero_points = b.ptr(op.consts["zero_points"], np.int32)


@lowers("qnn.concatenate")
def _qnn_concatenate(b: NodeBuilder, n, op: PlanOp) -> None:
    n.kind = KINDS[op.op]
    ca = n.attrs.concat
    ca.axis = op.attrs["axis"]
    ca.n = len(b.ins)
    for k, pl in enumerate(op.attrs["inputs"]):
        ca.requant[k] = pl["requant"]
        fill_rq_tensor(ca.rq[k], pl["mode"], pl["multiplier"], pl["shift"], pl["input_zero_point"],
                       pl["output_zero_point"])


@lowers("qnn.leaky_relu")
def _qnn_leaky_relu(b: NodeBuilder, n, op: PlanOp) -> None:
    n.kind = KINDS[op.op]
    la, a = n.attrs.leaky_relu, op.attrs
    fill_rq_tensor(la.rq, a["mode"], a["multiplier"], a["shift"], a["input_zero_point"], a["output_zero_point"])
    la.upcast = a["upcast"]
    la.input_zero_point, la.output_zero_point = a["input_zero_point"], a["output_zero_point"]
    la.alpha_multiplier, la.alpha_shift = a["alpha_multiplier"], a["alpha_shift"]
    la.zp_multiplier, la.zp_shift = a["zp_multiplier"], a["zp_shift"]


@lowers(*_qnn.UNARY_OPS)
def _lookup(b: NodeBuilder, n, op: PlanOp) -> None:
    n.kind = KINDS["lookup"]
    a = op.attrs
    table = _legalize.build_table(b.lib, op.op, op.out.dtype, a["in_scale"], a["in_zero_point"], a["out_scale"],
                                  a["out_zero_point"], b.m.device, b.stream)
    b.m._keep.append(table)
    b.m.tables[op.name] = table
    n.ext[0] = table.data_ptr()


@lowers("qnn.simulated_quantize", "qnn.simulated_dequantize")
def _simulated(b: NodeBuilder, n, op: PlanOp) -> None:
    n.kind = KINDS[op.op]
    sq, a = n.attrs.simq, op.attrs
    sq.axis, sq.n_scales, sq.n_zero_points = a["axis"], a["n_scales"], a["n_zero_points"]
    # each parameter is a folded constant uploaded here or a graph tensor's buffer
    # (read on the device when the node runs)
    src = {key: b.ptr(op.consts[key]) if k < 0 else b.m.buffers[op.inputs[k]].data_ptr()
           for key, k in a["sources"].items()}
    sq.dtype_code, sq.scales, sq.zero_points = src["dtype_code"], src["scales"], src["zero_points"]


@lowers("transpose")
def _transpose(b: NodeBuilder, n, op: PlanOp) -> None:
    n.kind = KINDS["transpose"]
    n.attrs.transpose = transpose_attrs(op.attrs["axes"])


@lowers("nn.bias_add")
def _bias_add(b: NodeBuilder, n, op: PlanOp) -> None:
    n.kind = KINDS["nn.bias_add"]
    n.attrs.bias_add.axis = op.attrs["axis"]


@lowers("clip", "nn.relu")
def _clip(b: NodeBuilder, n, op: PlanOp) -> None:
    n.kind = KINDS["clip"]
    n.attrs.clip.a_min, n.attrs.clip.a_max = op.attrs["lo"], op.attrs["hi"]


@lowers("nn.max_pool2d", "nn.avg_pool2d")
def _pool2d(b: NodeBuilder, n, op: PlanOp) -> None:
    n.kind = KINDS[op.op]
    if op.name in b.pool_names:
        b.ensure_shadow(op.inputs[0])
        n.ext[0] = b.shadow_bufs[op.inputs[0]].data_ptr()
        if op.name in b.shadow_bufs:
            b.shadow_out(n, op.name)
    pa, a = n.attrs.pool2d, op.attrs
    for field in ("pool_size", "strides", "padding", "dilation"):
        getattr(pa, field)[:] = list(a[field])
    pa.count_include_pad = int(a.get("count_include_pad", False))


@lowers("nn.batch_flatten", "reshape", "annotation.stop_fusion", "annotation.cast_hint")
def _copy(b: NodeBuilder, n, op: PlanOp) -> None:
    n.kind = KINDS["copy"]


@lowers("cast", "nn.global_avg_pool2d", "nn.dense")
def _no_attrs(b: NodeBuilder, n, op: PlanOp) -> None:
    n.kind = KINDS["dense_f32" if op.op == "nn.dense" else op.op]  # float32 (an int8 one is a qnn.dense)


@lowers("nn.conv2d")
def _conv2d_f32(b: NodeBuilder, n, op: PlanOp) -> None:
    """float32 (int8 ones are lowered to qnn.conv2d)"""
    n.kind = KINDS["conv2d_f32"]
    conv_attrs(n.attrs.conv2d, op.attrs, op.consts)


@lowers("nn.pad")
def _pad(b: NodeBuilder, n, op: PlanOp) -> None:
    n.kind = KINDS["nn.pad"]
    pa, a = n.attrs.pad, op.attrs
    for d, (before, after) in enumerate(a["pad_width"]):
        pa.before[d], pa.after[d] = before, after
    if op.out.dtype == "float32":
        pa.value_f = float(a["value"])
    else:
        pa.value_i = int(a["value"])


@lowers("ewise")
def _ewise(b: NodeBuilder, n, op: PlanOp) -> None:
    n.kind = KINDS["ewise"]
    ew, a = n.attrs.ewise, op.attrs
    ew.op, ew.rhs_kind = _lib.TK_EW[a["ew"]], a["rhs_kind"]
    ew.scalar_f, ew.scalar_i = a.get("scalar_f", 0.0), a.get("scalar_i", 0)
    ew.lo, ew.hi = a.get("lo", 0.0), a.get("hi", 0.0)
    ew.multiplier, ew.shift = a.get("multiplier", 0), a.get("shift", 0)
