"""Pass groups (mi_pass_group, execute_stage in h264decode_amd/csrc/mi_batch.cpp): the entropy stages of G consecutive passes are released together,
behind the reconstruction of every pass before the group.  CPU tests: the plan through the hooks entry, and a small model of the event graph that
execute_stage enqueues -- one entropy node E(p) and one reconstruction node R(p) per pass, an edge for every hipStreamWaitEvent and for stream order --
over pass sequences with G in {0, 2, 3}, the plan changing mid-sequence and an exclusive (serialised) pass in the middle."""
import ctypes
import itertools

import pytest

MI_SETS = 3
SHIPPED_G = 2  # MI_PASS_GROUP_DEFAULT


def _plan(H, n_slices0, capacity, pics_per_launch, has_b):
    return H.load_hooks().h264mi_internal_pass_group_plan(n_slices0, capacity, pics_per_launch, has_b)


def test_plan_table(H):
    cap = 256 * 4 * 6  # the chip's CUs x SIMDs x wavefronts of k_entropy_m per SIMD
    assert cap == 6144
    assert _plan(H, 7680, cap, 256, 0) == SHIPPED_G  # the bench shape: 256 streams x 30 pictures of one slice
    assert _plan(H, 960, cap, 32, 0) == 0 and _plan(H, 960, cap, 256, 0) == 0
    assert _plan(H, 300, cap, 10, 0) == 0 and _plan(H, 300, cap, 256, 0) == 0
    assert _plan(H, cap, cap, 256, 0) == 0  # exactly at capacity: no second round
    assert _plan(H, cap + 1, cap, 256, 0) == SHIPPED_G
    for n, pics in itertools.product((1, 300, 960, cap, cap + 1, 7680, 100000), (1, 32, 128, 129, 256, 4096)):
        assert _plan(H, n, cap, pics, 1) == 0, "a batch with B slices is never grouped"
        g = _plan(H, n, cap, pics, 0)
        assert g in (0, SHIPPED_G) and g <= MI_SETS
        assert (g != 0) == (n > cap), (n, pics)  # pictures per launch decide nothing: no measurement has shown banded launches losing
    assert _plan(H, 7680, 0, 256, 0) == 0  # no device properties: ungrouped


def test_hooks_entries_refuse_nonsense(H):
    h = H.load_hooks()
    assert h.h264mi_internal_set_pass_group(None, 2) == -1  # H264MI_EINVAL
    a = ctypes.c_int64()
    assert h.h264mi_internal_pass_waits(None, ctypes.byref(a), ctypes.byref(a)) == -1


# ---- the event graph.  A pass is (G, serial): G the plan of its batch (forced or not), serial: profiling or exclusive -- the serialised path.
class Model:
    """What execute_stage keeps between passes, and the waits it enqueues, restated: nodes ("E", p) / ("R", p), edges before -> after."""

    def __init__(self):
        self.p = 0
        self.group_left, self.gate = 0, None  # gate: the pass whose ev_rec the open group waits for
        self.last_rec = None                  # the pass that recorded an ev_rec last
        self.rec_of_set = {}                  # set -> pass whose ev_rec / ev_col record is the latest of that set
        self.stream_tail = {}                 # stream -> last node enqueued on it
        self.edges, self.nodes = set(), []
        self.waits = {}                       # pass -> {"set": p - MI_SETS or None, "gate": pass or None}
        self.passes = []

    def _on_stream(self, stream, node):
        if stream in self.stream_tail:
            self.edges.add((self.stream_tail[stream], node))
        self.stream_tail[stream] = node

    def execute(self, G, serial=False, exclusive=False):
        if exclusive:  # the caller has drained every stream; the pass moves to record set 0
            self.p += (MI_SETS - self.p % MI_SETS) % MI_SETS
            serial = True
        p, s = self.p, self.p % MI_SETS
        E, R = ("E", p), ("R", p)
        self.nodes += [E, R]
        if serial or G <= 0:
            self.group_left = 0
        else:
            if self.group_left <= 0:
                self.group_left, self.gate = min(G, MI_SETS), self.last_rec
            self.group_left -= 1
        gated = (not serial) and G > 0 and self.gate is not None
        w = {"set": None, "gate": self.gate if gated else None}
        if serial:  # both stages on the caller's stream, which has waited for every earlier ev_rec
            self._on_stream("user", E)
            self._on_stream("user", R)
        else:
            es = "ent%d" % (p & 1)
            if p >= MI_SETS and s in self.rec_of_set:
                w["set"] = self.rec_of_set[s]
                self.edges.add((("R", w["set"]), E))
                self.edges.add((("E", w["set"]), E))  # ev_col
            if gated:
                self.edges.add((("R", self.gate), E))
            self._on_stream(es, E)
            self.edges.add((E, R))  # ev_ent
            self._on_stream("rec", R)
            self._on_stream("user", R)  # the caller's stream waits for ev_rec
        self.rec_of_set[s] = p
        self.last_rec = p
        self.waits[p] = w
        self.passes.append((p, G, serial))
        self.p += 1


def _topological(nodes, edges):
    indeg = {n: 0 for n in nodes}
    out = {n: [] for n in nodes}
    for a, b in edges:
        out[a].append(b)
        indeg[b] += 1
    ready = [n for n in nodes if indeg[n] == 0]
    order = []
    while ready:
        n = ready.pop()
        order.append(n)
        for m in out[n]:
            indeg[m] -= 1
            if indeg[m] == 0:
                ready.append(m)
    return order if len(order) == len(nodes) else None


def _reaches(edges, a, b):
    out = {}
    for x, y in edges:
        out.setdefault(x, []).append(y)
    seen, todo = {a}, [a]
    while todo:
        for y in out.get(todo.pop(), []):
            if y == b:
                return True
            if y not in seen:
                seen.add(y)
                todo.append(y)
    return False


SEQUENCES = {
    "g0": [(0, False, False)] * 9,
    "g2": [(2, False, False)] * 9,
    "g3": [(3, False, False)] * 10,
    "plan_changes": [(2, False, False)] * 3 + [(3, False, False)] * 4 + [(0, False, False)] * 2 + [(2, False, False)] * 3 + [(3, False, False)] + [(2, False, False)] * 2,
    "exclusive_in_the_middle_g2": [(2, False, False)] * 4 + [(2, True, True)] + [(2, False, False)] * 5,
    "exclusive_in_the_middle_g3": [(3, False, False)] * 5 + [(3, True, True)] + [(3, False, False)] * 7,
    "profiling_between_groups": [(3, False, False)] * 3 + [(3, True, False)] * 2 + [(3, False, False)] * 4,
    "ungrouped_pass_closes_the_group": [(3, False, False)] * 4 + [(0, False, False)] + [(3, False, False)] * 5,
}


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_event_graph(name):
    m = Model()
    for G, serial, exclusive in SEQUENCES[name]:
        m.execute(G, serial, exclusive)
    order = _topological(m.nodes, m.edges)
    assert order is not None, "a cycle: the passes would wait for each other"
    executed = [p for p, _, _ in m.passes]
    groups = []  # runs of consecutive gated-or-opening grouped passes, as the model's state saw them
    left = 0
    for p, G, serial in m.passes:
        w = m.waits[p]
        # set reuse is as safe as it was: the entropy launch is behind the reconstruction (and the entropy stream) of the set's previous user
        prev = [q for q in executed if q < p and q % MI_SETS == p % MI_SETS]
        if prev:
            assert _reaches(m.edges, ("R", prev[-1]), ("E", p)), (name, p, "not ordered behind the pass that used its record set")
            assert _reaches(m.edges, ("E", prev[-1]), ("E", p))
        if w["gate"] is not None:
            assert w["gate"] < p and w["gate"] in executed, "a gate names a strictly earlier pass"
        if serial or G <= 0:
            assert w["gate"] is None
            left = 0
            continue
        if left <= 0:
            left = min(G, MI_SETS)
            groups.append([])
        left -= 1
        groups[-1].append(p)
    for grp in groups:
        gates = {m.waits[p]["gate"] for p in grp}
        assert len(gates) == 1, (name, grp, "every pass of a group carries the same gate")
        gate = gates.pop()
        first = grp[0]
        before = [q for q in executed if q < first]
        assert gate == (before[-1] if before else None), "the gate is the last pass executed before the group opened"
        assert len(grp) <= MI_SETS
        for p in grp:  # the whole group starts behind the reconstruction of every earlier pass
            for q in before:
                assert _reaches(m.edges, ("R", q), ("E", p)), (name, q, p)
        # the gate's event is still the gate pass's record when the group's last pass enqueues its wait: nobody in between recorded that set's ev_rec
        if gate is not None:
            assert not [q for q in executed if gate < q < grp[-1] and q % MI_SETS == gate % MI_SETS], (name, grp, gate)


def test_g0_wait_set_is_todays():
    m = Model()
    for _ in range(8):
        m.execute(0)
    for p in range(8):
        assert m.waits[p] == {"set": p - MI_SETS if p >= MI_SETS else None, "gate": None}
    # ... and the same edges as a model that knows nothing of groups
    want = set()
    for p in range(8):
        if p >= MI_SETS:
            want |= {(("R", p - MI_SETS), ("E", p)), (("E", p - MI_SETS), ("E", p))}
        if p >= 2:
            want.add((("E", p - 2), ("E", p)))  # the entropy streams alternate
        if p >= 1:
            want.add((("R", p - 1), ("R", p)))
        want.add((("E", p), ("R", p)))
    assert m.edges == want


def test_groups_form_as_drawn():
    """E0 E1 | R0 R1 | E2 E3 ...: with G = 2 passes 2k and 2k + 1 wait for R(2k - 1); with G = 3 passes 3k .. 3k + 2 wait for R(3k - 1)."""
    for G in (2, 3):
        m = Model()
        for _ in range(4 * G + 1):
            m.execute(G)
        for p in range(4 * G + 1):
            first = p - p % G
            assert m.waits[p]["gate"] == (first - 1 if first else None), (G, p)
