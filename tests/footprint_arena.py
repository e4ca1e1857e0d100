"""A guarded arena for one call of the C ABI: every device buffer of the call -- inputs, outputs, optional outputs, the
workspace -- is carved out of ONE allocation the test owns, with a guard band before and after each, so that what a kernel
writes outside a payload lands in memory the test looks at, and what it fails to write is told from what it wrote.

  * the whole arena is filled with F64_POISON, one quiet-NaN bit pattern, before anything else; the payload of an int32
    output with I32_POISON (above any max_iter a test uses), of a byte output with U8_POISON (the flag encoding of
    include/diffqcqp_hip.h knows 0, 1, 2);  doubles are compared as int64, never as floating point;
  * inputs are copied in over the poison, and a pristine copy of the whole arena is kept: a guard or an input is intact
    when its bytes still equal the copy's;
  * a guard is at least twice g x (bytes per problem of its buffer) and at least 4 KiB, g the problems per workgroup of the
    route (tests/footprint_cases.py): a whole rounded-up tile of overrun stays inside the arena;  the workspace's unit is
    not a problem: its guards (in front and behind, and it is the last buffer) hold a tile of work-list entries (2 g ints)
    plus the larger of the whole scratch the call was given and twice one workgroup's scratch slice (general_any.hip:
    any_fwd_stride / any_bwd_stride doubles, one slice per workgroup of any_grid), so that a scratch sized for fewer or
    smaller slices than the kernel uses is caught inside the arena;
  * sliced=True places every payload one problem past a 512-byte boundary -- the alignment of `t[1:]` of a torch tensor,
    8 bytes only for odd N --, sliced=False on the boundary itself; the workspace ("ws": exactly the bytes asked for, its
    work-list zeroed as ops.make_workspace does, the scratch behind it left poisoned) always sits on a boundary.
Works on CPU tensors too (tests/test_footprint_cases.py proves there that every check can fail)."""
import torch

F64_POISON = 0x7FF8DEADBEEFCAFE   # quiet NaN, payload 0xDEADBEEFCAFE
I32_POISON = 0x7F5A5A5A
U8_POISON = 0xA5
_POISON = {torch.float64: F64_POISON, torch.int32: I32_POISON, torch.uint8: U8_POISON}
_INT_VIEW = {torch.float64: torch.int64, torch.int32: torch.int32, torch.uint8: torch.uint8}
ALIGN = 512
MIN_GUARD = 4096
WORKLIST_ENTRY = 4   # bytes of a work-list entry (an int: worklist.h kWsEntryInts)


def _up(n, a=ALIGN):
    return (n + a - 1) // a * a


def ws_guard(ws_bytes, worklist_bytes, slice_bytes, g):
    """The guard in front of and behind a workspace of ws_bytes, the first worklist_bytes of them the work-list, the rest
    scratch in slices of slice_bytes per workgroup."""
    return _up(max(MIN_GUARD, ws_bytes - worklist_bytes, 2 * slice_bytes) + 2 * g * WORKLIST_ENTRY)


class Arena:
    """specs: list of (name, role, dtype, shape, data).  role "in": `data` (a CPU tensor of that dtype and shape) is the
    payload; "out": poisoned, to be written by the call for every problem (shape[0] = B); "ws": shape = (bytes, bytes of
    the work-list in front), dtype uint8, `data` the bytes of one workgroup's scratch slice (0 or None: the call has no
    scratch).  shape[0] is the batch size, the rest one problem."""

    def __init__(self, specs, g, device, sliced=True):
        self.device = torch.device(device)
        self.bufs = {}
        self.order = []
        cursor, behind = 0, 0     # end of the last payload, the guard it wants behind it
        for name, role, dtype, shape, data in specs:
            esz = torch.empty((), dtype=dtype).element_size()
            per = esz
            for s in shape[1:]:
                per *= s
            nbytes = shape[0] if role == "ws" else shape[0] * per
            if role == "ws":
                guard = ws_guard(shape[0], shape[1], data or 0, g)
            else:
                guard = _up(max(MIN_GUARD, 2 * g * per))
            off = _up(cursor + max(guard, behind)) + (per if (sliced and role != "ws") else 0)
            self.bufs[name] = dict(role=role, dtype=dtype, shape=tuple(shape), off=off, nbytes=nbytes, per=per, esz=esz,
                                   hi=off + nbytes, guard=guard)
            self.order.append(name)
            cursor, behind = off + nbytes, guard
        self.total = _up(cursor + behind)
        self.raw = torch.empty(self.total, dtype=torch.uint8, device=self.device)
        self.raw.view(torch.int64).fill_(F64_POISON)
        for name, role, dtype, shape, data in specs:
            b = self.bufs[name]
            if role == "in":
                self.view(name).copy_(data.reshape(shape))
            elif role == "ws":
                self.raw[b["off"]: b["off"] + shape[1]].zero_()
            elif dtype != torch.float64 and b["nbytes"]:
                self.view(name).fill_(_POISON[dtype])
        self.pristine = self.raw.clone()

    # ---- access
    def view(self, name):
        b = self.bufs[name]
        if b["role"] == "ws":
            return self.raw[b["off"]: b["off"] + b["nbytes"]]
        return self.raw[b["off"]: b["off"] + b["nbytes"]].view(b["dtype"]).view(b["shape"])

    def ptr(self, name):
        return self.raw.data_ptr() + self.bufs[name]["off"]

    def window(self, name, before=0, after=0):
        """The payload as a flat tensor of its dtype with `before` / `after` elements of its guards around it (for the
        fake kernels of the CPU test)."""
        b = self.bufs[name]
        return self.raw[b["off"] - before * b["esz"]: b["off"] + b["nbytes"] + after * b["esz"]].view(b["dtype"])

    # ---- checks (each raises AssertionError naming the buffer and the offset)
    def _first_diff(self, lo, hi):
        if lo >= hi or torch.equal(self.raw[lo:hi], self.pristine[lo:hi]):
            return None
        return lo + int((self.raw[lo:hi] != self.pristine[lo:hi]).nonzero()[0, 0])

    def check_guards(self):
        """Every byte outside the payloads still holds its sentinel."""
        edges = [(self.bufs[n]["off"], self.bufs[n]["hi"], n) for n in self.order]
        lo, prev = 0, None
        for off, hi, name in edges + [(self.total, self.total, None)]:
            at = self._first_diff(lo, off)
            if at is not None:
                # the nearer payload names the finding: bytes behind `prev` or in front of `name`
                if prev is not None and (name is None or at - self.bufs[prev]["hi"] < off - at):
                    raise AssertionError("guard behind '%s' overwritten: byte %d past the end of its payload (arena offset %d)"
                                         % (prev, at - self.bufs[prev]["hi"], at))
                raise AssertionError("guard in front of '%s' overwritten: byte %d before its payload (arena offset %d)"
                                     % (name, off - at, at))
            lo, prev = hi, name

    def check_inputs(self):
        for name in self.order:
            b = self.bufs[name]
            if b["role"] == "in":
                at = self._first_diff(b["off"], b["hi"])
                assert at is None, "input '%s' modified at byte offset %d (element %d)" % (name, at - b["off"], (at - b["off"]) // b["esz"])

    def check_written(self, name, rows=None):
        """No sentinel left in the output `name` (rows: a bool mask over the problems, default all)."""
        b = self.bufs[name]
        assert b["role"] == "out"
        if b["nbytes"] == 0:
            return
        v = self.view(name).view(_INT_VIEW[b["dtype"]]).reshape(b["shape"][0], -1)
        left = v == _POISON[b["dtype"]]
        if rows is not None:
            left = left & rows.to(left.device).reshape(-1, 1)
        if bool(left.any()):
            prob, el = [int(i) for i in left.nonzero()[0]]
            raise AssertionError("output '%s' not written: problem %d of %d, element %d (offset %d) still holds the sentinel"
                                 % (name, prob, b["shape"][0], el, prob * v.shape[1] + el))

    def check_untouched(self):
        at = self._first_diff(0, self.total)
        assert at is None, "arena modified at offset %d" % at

    def check_pristine(self, name, nbytes=None):
        """The first nbytes (default: all) of the payload `name` are what they were before the call: an output the call was
        not handed (its pointer NULL), or the work-list in front of a scratch that a call documents as not touched."""
        b = self.bufs[name]
        at = self._first_diff(b["off"], b["off"] + (b["nbytes"] if nbytes is None else nbytes))
        assert at is None, "'%s' modified at byte offset %d" % (name, at - b["off"])


# ---- the buffers of a call of the C ABI (include/diffqcqp_hip.h; argument orders as in diffqcqp_amd/ops.py)
F64, I32, U8 = torch.float64, torch.int32, torch.uint8
_AUX = {"qp": (), "qcqp": ("l_n", "mu"), "box": ("l_min", "l_max"), "sbox": ("l_min", "l_max", "v")}


def call_specs(pas, kind, N, B, layout, d, ws_bytes, worklist_bytes, slice_bytes=0):
    """The specs of every buffer of one call, every optional output requested.  d: the inputs as CPU tensors of B problems
    (P already (B,N) for DQQ_P_DIAG; the backward's x among them); slice_bytes: one workgroup's share of the scratch."""
    pshape = (B, N) if (layout & 0xff) == 2 else (B, N, N)
    half = (B, N // 2, 1)
    specs = [("P", "in", F64, pshape, d["P"]), ("q", "in", F64, (B, N, 1), d["q"])]
    specs += [(n, "in", F64, half if kind == "qcqp" else (B, N, 1), d[n]) for n in _AUX[kind]]
    if pas == 0:
        specs += [("x", "out", F64, (B, N, 1), None), ("iters", "out", I32, (B,), None),
                  ("pdiag_out", "out", F64, (B, N), None), ("diag_flags_out", "out", U8, (B,), None)]
    else:
        specs += [("x", "in", F64, (B, N, 1), d["x"]), ("grad_x", "in", F64, (B, N, 1), d["grad_x"]),
                  ("grad_P", "out", F64, pshape, None), ("grad_q", "out", F64, (B, N, 1), None)]
        if kind == "qcqp":
            specs += [(n, "out", F64, half, None) for n in ("grad_l_n", "grad_mu", "gamma", "dgamma")]
        elif kind == "box":
            specs += [("grad_l_min", "out", F64, (B, N, 1), None), ("grad_l_max", "out", F64, (B, N, 1), None),
                      ("gamma", "out", F64, (B, 2 * N), None), ("dgamma", "out", F64, (B, 2 * N), None)]
        specs += [("ir_steps", "out", I32, (B, 2) if kind == "box" else (B,), None)]
    return specs + [("ws", "ws", U8, (ws_bytes, worklist_bytes), slice_bytes)]


def run_call(lib, a, pas, kind, N, B, layout, stream, eps=1e-7, max_iter=1000, mu_prox=1e-7, epsilon=1e-10):
    """The call, straight through the C ABI with pointers into the arena `a`; no report word, no diagonal cache.  -> rc"""
    p = a.ptr
    ws = (p("ws"), a.bufs["ws"]["nbytes"], stream)
    if pas == 0:
        tail = (p("x"), B, N, eps, mu_prox, max_iter, 1, layout, p("iters"), p("pdiag_out"), p("diag_flags_out")) + ws
        if kind == "qp":
            return lib.dqq_qp_fwd_f64(p("P"), p("q"), *tail)
        if kind == "qcqp":
            return lib.dqq_qcqp_fwd_f64(p("P"), p("q"), p("l_n"), p("mu"), *tail)
        if kind == "box":
            return lib.dqq_boxqp_fwd_f64(p("P"), p("q"), p("l_min"), p("l_max"), *tail)
        return lib.dqq_signedboxqp_fwd_f64(p("P"), p("q"), p("l_min"), p("l_max"), p("v"), *tail)
    if kind == "qp":
        return lib.dqq_qp_bwd_f64(p("P"), p("q"), p("x"), p("grad_x"), p("grad_P"), p("grad_q"), B, N, epsilon, layout,
                                  p("ir_steps"), None, None, None, *ws)
    if kind == "qcqp":
        return lib.dqq_qcqp_bwd_f64(p("P"), p("q"), p("l_n"), p("mu"), p("x"), p("grad_x"), p("grad_P"), p("grad_q"),
                                    p("grad_l_n"), p("grad_mu"), p("gamma"), p("dgamma"), B, N, epsilon, layout, p("ir_steps"),
                                    None, None, None, *ws)
    return lib.dqq_boxqp_bwd_f64(p("P"), p("q"), p("l_min"), p("l_max"), p("x"), p("grad_x"), p("grad_P"), p("grad_q"),
                                 p("grad_l_min"), p("grad_l_max"), p("gamma"), p("dgamma"), B, N, epsilon, layout, p("ir_steps"),
                                 None, None, *ws)


def jvp_call_specs(kind, N, B, layout, d, ws_bytes=0, worklist_bytes=0, slice_bytes=0):
    """The specs of every buffer of one dqq_jvp_f64 call, ir_steps requested.  d: P (already (B,N) for DQQ_P_DIAG), q, the kind's
    extras, x and the tangents dP (P's shape), dq, and but for the QP da, db, as CPU tensors of B problems -- all inputs.  A
    workspace only when ws_bytes > 0 (JvpAny: the work-list in front, the backward's scratch behind it)."""
    pshape = (B, N) if (layout & 0xff) == 2 else (B, N, N)
    eshape = (B, N // 2, 1) if kind == "qcqp" else (B, N, 1)
    specs = [("P", "in", F64, pshape, d["P"]), ("q", "in", F64, (B, N, 1), d["q"])]
    specs += [(n, "in", F64, eshape, d[n]) for n in _AUX[kind]]
    specs += [("x", "in", F64, (B, N, 1), d["x"]), ("dP", "in", F64, pshape, d["dP"]), ("dq", "in", F64, (B, N, 1), d["dq"])]
    if kind != "qp":
        specs += [("da", "in", F64, eshape, d["da"]), ("db", "in", F64, eshape, d["db"])]
    specs += [("dx", "out", F64, (B, N, 1), None), ("ir_steps", "out", I32, (B, 2) if kind in ("box", "sbox") else (B,), None)]
    return specs + ([("ws", "ws", U8, (ws_bytes, worklist_bytes), slice_bytes)] if ws_bytes else [])


def run_jvp(lib, a, kind, N, B, layout, stream, epsilon=1e-10, steps=True, only_dq=False, ws_short=0):
    """The call, with pointers into the arena `a`.  steps=False: ir_steps = NULL; only_dq: every tangent but dq NULL; ws_short:
    that many bytes less of workspace are declared than the arena holds.  -> rc"""
    p = a.ptr
    k = {"qp": 0, "qcqp": 1, "box": 2, "sbox": 3}[kind]
    ex = [p(n) for n in _AUX[kind]] + [None] * (3 - len(_AUX[kind]))
    tan = [None if only_dq else p("dP"), p("dq")] + ([None, None] if (kind == "qp" or only_dq) else [p("da"), p("db")])
    ws = (p("ws"), a.bufs["ws"]["nbytes"] - ws_short) if "ws" in a.bufs else (None, 0)
    return lib.dqq_jvp_f64(k, p("P"), p("q"), *ex, p("x"), *tan, p("dx"), B, N, epsilon, layout, p("ir_steps") if steps else None,
                           *ws, stream)
