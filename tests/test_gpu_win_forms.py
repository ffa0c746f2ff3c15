"""The k-mer stage over sliding windows, alone, against the oracle, with a launch witness.

kmcpg_kmers_device_windows runs what a lane runs for a staged piece of windows — k_window_desc (windows.hip), then K1 and the dedup stage
reading every window's bases in place — and hands out what they wrote.  For every case of the plan (tests/win_cases.py: windows that begin
and end on chunk, tile and lane seams, 1023 .. 3000 chunks for the one-workgroup scan, batches without a chunk or without a window, the
last k of the hash-once form and the first behind it, FracMinHash scales that leave chunks and windows empty, both sides of -u and -m,
slices that begin inside a read, more windows than the gather's grid holds, and the window view in every other K1 form) this

  * compares, bit for bit and without a tolerance, every hash (value, order, multiplicity), every NumKmers and every qlen with the
    oracle's generate_kmers on the window's text (sort_unique above -u, nothing below -m), and src and koff with the plan's own Python
    staging; a wrong hash in a window that matches nothing in any database fails here;
  * asserts that the witness (`Database.last_k1_launches()` / `last_k1_plan()`) names exactly the declared form and kernels, in order, with
    their template parameters, grids and block sizes, and for the list forms exactly what the first kernel left.

A closing test asserts that the four hash-once kernels and each form of the `view` group were witnessed.  tests/test_win_cases_cpu.py
checks the plan itself without a GPU.

Left out on purpose: the `hv != 0` rule (it would need a k-mer whose ntHash is zero; nobody has one); the grid-stride loop of the two chunk
passes (more than 262 144 chunks: the pieces the library cuts never hold that many); packed slices (stage() expands them before any window
kernel reads them: tests/test_gpu_pack.py, tests/test_gpu_sliding.py).
"""
import numpy as np
import pytest

from tests import win_cases as P
from tests.test_gpu_k1_forms import _Env

pytestmark = pytest.mark.gpu

_dbs = {}
_witnessed = set()   # kernel names over the module
_forms = set()       # forms of the view group's plans
_done = set()
_refs = {}           # case id -> the oracle's lists per piece: computed once, never changed


def _db(key):
    from kmcp_amd import Database, lib
    if key not in _dbs:
        spec = lib.SynthSpec(k=key.k, num_hashes=1, fpr=0.3, n_blocks=1, cols_per_block=8, num_sigs=1000, kmers_per_col=10, seed=1, scale=key.scale,
                             syncmer_s=key.ws if key.mode == "syn" else 0, minimizer_w=key.ws if key.mode == "min" else 0)
        db = Database.open_synthetic(spec)
        db.set_profiling(1)
        _dbs[key] = db
    return _dbs[key]


@pytest.fixture(scope="module", autouse=True)
def _close_databases():
    yield
    while _dbs:
        _dbs.popitem()[1].close()


def _run(db, c, st):
    """one call on one staged piece -> (hashes, koff, src, nk, qlen) as the device left them"""
    import torch
    from kmcp_amd import default_params, lib
    dev = torch.device("cuda:0")
    text = np.full(st.sb + 16, 0xA5, dtype=np.uint8)   # (what lies behind the staged text must not matter)
    text[:st.sb] = np.frombuffer(st.text, dtype=np.uint8)
    t_text = torch.from_numpy(text).to(dev)
    t_pre = [torch.from_numpy(a.view(np.int64)).to(dev) for a in (st.soffs, st.wpre, st.vpre, st.cpre)]
    t_h = torch.full((st.bases + P.PAD_H,), P.FILL, dtype=torch.int64, device=dev)
    t_koff = torch.full((st.n_win + 1,), P.FILL, dtype=torch.int64, device=dev)
    t_src = torch.full((st.n_win + 1,), P.FILL, dtype=torch.int64, device=dev)
    t_nk = torch.full((st.n_win + 1,), P.FILL, dtype=torch.int32, device=dev)
    t_ql = torch.full((st.n_win + 1,), P.FILL, dtype=torch.int32, device=dev)
    p = default_params(min_qlen=c.min_qlen, min_matched=1, dedup_threshold=c.u)
    with _Env({}):
        db.kmers_device_windows(t_text.data_ptr(), *[t.data_ptr() for t in t_pre], st.n_slices, st.sb, st.n_chunks, st.n_win, st.bases, st.wmax,
                                lib.WindowSpec(c.step, c.window, int(c.greedy), 0), t_h.data_ptr(), t_h.numel(), t_koff.data_ptr(), t_src.data_ptr(),
                                t_nk.data_ptr(), t_ql.data_ptr(), params=p)
    torch.cuda.synchronize()
    return (t_h.cpu().numpy().view(np.uint64), t_koff.cpu().numpy().view(np.uint64), t_src.cpu().numpy().view(np.uint64), t_nk.cpu().numpy(),
            t_ql.cpu().numpy())


def _check_piece(c, n, st, ref, db):
    from kmcp_amd import lib
    what = "%s, call %d" % (c.id, n)
    try:
        h, koff, src, nk, ql = _run(db, c, st)
    except lib.KmcpGpuError as err:  # a device error is no mismatch: nothing more is started on a GPU that reported one
        pytest.exit("%s: %s" % (what, err), returncode=3)
    launches, plan = db.last_k1_launches(), db.last_k1_plan()
    _witnessed.update(w[0] for w in launches)
    if c.group == "view":
        _forms.add(plan["form"])
    problems = []
    e = c.expected(st)
    if launches != e["kernels"]:
        problems.append("launched %s, the plan declares %s" % (launches, e["kernels"]))
    left = None if c.left is None else c.left(c, st, ref)
    want_plan = dict(form=e["form"], codes_direct=e["codes_direct"], list_fallback=e["list_fallback"], adj_done=e["adj_done"], left_on_list=left)
    if plan != want_plan:
        problems.append("plan record %s, declared %s" % (plan, want_plan))
    problems += P.compare(st, ref, h, koff, src, nk, ql)   # every hash, count, qlen, src and koff; nothing behind the arrays' ends was touched
    assert not problems, "%s:\n" % what + "\n".join(problems[:12])


def _check_case(c, O):
    if c.id not in _refs:
        _refs[c.id] = [P.reference(c, st, O) for st in c.pieces()]
    db = _db(c.db)
    _done.add(c.id)
    for n, (st, ref) in enumerate(zip(c.pieces(), _refs[c.id])):
        _check_piece(c, n, st, ref, db)


@pytest.mark.parametrize("case", P.CASES, ids=[c.id for c in P.CASES])
def test_win_form(case, oracle_lib):
    _check_case(case, oracle_lib)


def test_refuses_bad_arguments(oracle_lib):
    """null pointers, a hash buffer below the windows' bases, a spec kmcpg_submit_windows refuses: KMCPG_EINVAL, before anything is launched"""
    import torch
    from kmcp_amd import lib
    c = [c for c in P.CASES if c.id == "pieces"][0]
    st = c.pieces()[1]
    db = _db(c.db)
    dev = torch.device("cuda:0")
    buf = torch.zeros(st.sb + st.bases + 64, dtype=torch.int64, device=dev)
    ptr = buf.data_ptr()
    good = [ptr, ptr, ptr, ptr, ptr, st.n_slices, st.sb, st.n_chunks, st.n_win, st.bases, st.wmax, lib.WindowSpec(c.step, c.window, 0, 0), ptr, st.bases, ptr, ptr, ptr, ptr]
    for i, bad in [(i, None) for i in (0, 1, 2, 3, 4, 12, 14, 15, 16, 17)] + [(13, st.bases - 1), (11, lib.WindowSpec(0, c.window, 0, 0)), (11, lib.WindowSpec(c.step, c.window, 2, 0)),
                                                                             (11, lib.WindowSpec(c.step, c.window, 0, 1)), (5, 0), (10, c.window + 1)]:
        args = list(good)
        args[i] = bad
        with pytest.raises(lib.KmcpGpuError) as err:
            db.kmers_device_windows(*args)
        assert err.value.code == -1, (i, str(err.value))   # KMCPG_EINVAL
    torch.cuda.synchronize()


def test_hash_once_kernels_and_view_forms_were_witnessed(oracle_lib):
    """over the module: the four hash-once kernels ran, and each form the view group names served a batch of windows (cases that were
    deselected run here)"""
    for c in P.CASES:
        if c.id not in _done:
            _check_case(c, oracle_lib)
    assert set(P.WIN_ONCE) <= _witnessed, sorted(set(P.WIN_ONCE) - _witnessed)
    assert _forms == set(P.VIEW_FORMS), (sorted(_forms), P.VIEW_FORMS)
