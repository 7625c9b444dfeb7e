"""The host add paths of the replay ring (rb_add, rb_add_particles, rb_add_records) on an MI355X,
bit for bit against a numpy model of the ring, through each of the three routes the staged records
can take into HBM (replay.hip push_staged): in the kernel arguments, by the put kernel out of the
mapped staging buffer, and by chunked copies.  Every case starts with ptr mid-ring so the write wraps.
The device adds are tested against these host adds (test_gpu_device_rollout.py and its neighbours).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PUT_ARG_FLOATS = 960            # replay.hip kPutArgFloats
PUT_KERNEL_BYTES = 256 << 10    # replay.hip kPutKernelBytes

FEATURED = [(17, 6), (3, 1)]                        # (state_dim, action_dim)
PARTICLES = [(7, 16, 9, 3), (3, 5, 3, 2)]           # (feat_dim, n_particles, particle_dim, action_dim)
SHAPES = FEATURED + PARTICLES


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def _widths(shape):
    """The flat field widths of a record, in the order of the add arguments (done last)."""
    if len(shape) == 2:
        sd, ad = shape
        return (sd, ad, sd, 1, 1)
    F, N, D, A = shape
    return (F, N * D, A, F, N * D, 1, 1)


def _rec(shape):
    return (sum(_widths(shape)) + 3) // 4 * 4


def _route(n, cap, rec):
    """The route n records take (only the last `cap` of them are written)."""
    n = min(n, cap)
    if n * rec <= PUT_ARG_FLOATS:
        return "args"
    return "put" if n * rec * 4 <= PUT_KERNEL_BYTES else "memcpy"


class _Model:
    """cap rows of rec floats, written one row at a time at ptr (wrapping): float32 of the float64
    input, not_done = 1 - done in the last field, a zero pad behind it."""

    def __init__(self, shape, cap):
        self.widths = _widths(shape)
        self.cap, self.ptr, self.size = cap, 0, 0
        self.data = np.zeros((cap, _rec(shape)), dtype=np.float32)

    def add(self, arrays):
        n = arrays[0].shape[0]
        cols = [np.asarray(x, dtype=np.float64).reshape(n, w) for x, w in zip(arrays, self.widths)]
        cols[-1] = 1.0 - cols[-1]
        rows = np.concatenate(cols, axis=1).astype(np.float32)
        for row in rows:
            self.data[self.ptr, :rows.shape[1]] = row
            self.ptr = (self.ptr + 1) % self.cap
            self.size = min(self.size + 1, self.cap)


def _ring(shape, cap):
    from td3_amd.my_replay_buffer import ReplayBuffer_featured, ReplayBuffer_particles
    if len(shape) == 2:
        rb = ReplayBuffer_featured(Box((shape[0],)), Box((shape[1],)), max_size=cap)
    else:
        F, N, D, A = shape
        rb = ReplayBuffer_particles((Box((F,)), Box((N, D))), Box((A,)), max_size=cap)
    assert rb.record_floats == _rec(shape)
    return rb, _Model(shape, cap)


def _rows(rs, shape, n):
    """n float64 transitions whose values fp32 does not hold exactly (both sides round them once)."""
    out = []
    for w in _widths(shape):
        out.append(rs.standard_normal((n, w)))
    out[-2] = out[-2].reshape(n)
    out[-1] = (rs.uniform(size=n) < 0.3).astype(np.float64)
    assert not np.array_equal(out[0], out[0].astype(np.float32).astype(np.float64))
    return out


def _add_batch(rb, model, shape, rows):
    if len(shape) == 4:                                  # the particle blocks as the API's [n][N][D]
        n = rows[0].shape[0]
        rows = list(rows)
        rows[1] = rows[1].reshape(n, shape[1], shape[2])
        rows[4] = rows[4].reshape(n, shape[1], shape[2])
    rb.add_batch(*rows)
    model.add(rows)


def _add_one(rb, model, shape, rows, i):
    """Transition i of `rows` through the per-step add()."""
    one = [x[i] for x in rows]
    if len(shape) == 2:
        s, a, s2, r, d = one
        rb.add(s, a, s2, r, d)
    else:
        f, p, a, f2, p2, r, d = one
        nd = (shape[1], shape[2])
        rb.add((f, p.reshape(nd)), a, (f2, p2.reshape(nd)), r, d)
    model.add([x[i:i + 1] for x in rows])


def _same(rb, model):
    assert (rb.ptr, rb.size) == (model.ptr, model.size)       # reading ptr flushes what add() staged
    np.testing.assert_array_equal(rb._records(), model.data)


@pytest.mark.parametrize("shape", SHAPES)
def test_add_and_flush_take_the_arguments_route(shape):
    """One add() + flush() in the last-but-one row, then three add() + one flush() that wrap."""
    cap, rec = 12, _rec(shape)
    rb, model = _ring(shape, cap)
    rs = np.random.RandomState(1)
    _add_batch(rb, model, shape, _rows(rs, shape, cap - 2))
    assert model.ptr == cap - 2
    rows = _rows(rs, shape, 4)
    assert _route(1, cap, rec) == "args" and _route(3, cap, rec) == "args"
    _add_one(rb, model, shape, rows, 0)
    rb.flush()
    _same(rb, model)
    for i in (1, 2, 3):
        _add_one(rb, model, shape, rows, i)
    rb.flush()
    _same(rb, model)
    assert (model.ptr, model.size) == (2, cap)


@pytest.mark.parametrize("shape,n", [((17, 6), 36), ((3, 1), 96), ((7, 16, 9, 3), 36), ((3, 5, 3, 2), 36)])
def test_add_batch_takes_the_put_kernel_route(shape, n):
    """A few dozen rows (more of the 12-float record, to pass kPutArgFloats), 10 rows before the end."""
    cap, rec = n + 20, _rec(shape)
    rb, model = _ring(shape, cap)
    rs = np.random.RandomState(2)
    _add_batch(rb, model, shape, _rows(rs, shape, cap - 10))
    assert model.ptr == cap - 10
    assert _route(n, cap, rec) == "put"
    _add_batch(rb, model, shape, _rows(rs, shape, n))
    _same(rb, model)
    assert (model.ptr, model.size) == (n - 10, cap)


@pytest.mark.parametrize("shape,cap,ptr,n", [((17, 6), 2000, 500, 1600), ((3, 1), 6000, 1000, 5500),
                                             ((7, 16, 9, 3), 256, 30, 240), ((3, 5, 3, 2), 2000, 500, 1700)])
def test_add_batch_takes_the_memcpy_route_in_two_chunks(shape, cap, ptr, n):
    """Just over kPutKernelBytes and below cap: the copy to the end of the ring, then the rest."""
    rec = _rec(shape)
    rb, model = _ring(shape, cap)
    rs = np.random.RandomState(3)
    _add_batch(rb, model, shape, _rows(rs, shape, ptr))
    assert model.ptr == ptr
    assert n < cap and _route(n, cap, rec) == "memcpy" and ptr + n > cap
    _add_batch(rb, model, shape, _rows(rs, shape, n))
    _same(rb, model)
    assert (model.ptr, model.size) == (ptr + n - cap, cap)


@pytest.mark.parametrize("shape,route", [((17, 6), "args"), ((3, 1), "args"), ((7, 16, 9, 3), "put"),
                                         ((3, 5, 3, 2), "args")])
def test_add_batch_past_capacity_keeps_the_last_rows(shape, route):
    """n = 25 into a 10-row ring at ptr 4: the last 10 rows survive, where 25 single adds put them."""
    cap, n, rec = 10, 25, _rec(shape)
    rb, model = _ring(shape, cap)
    rs = np.random.RandomState(4)
    _add_batch(rb, model, shape, _rows(rs, shape, 4))
    assert _route(n, cap, rec) == route
    _add_batch(rb, model, shape, _rows(rs, shape, n))
    _same(rb, model)
    assert (model.ptr, model.size) == ((4 + n) % cap, cap)


@pytest.mark.parametrize("shape,stage,cap", [((17, 6), 4096, 1000), ((3, 1), 4096, 4100),
                                             ((7, 16, 9, 3), 256, 260), ((3, 5, 3, 2), 256, 100)])
def test_add_past_the_stage_length_flushes_itself(shape, stage, cap):
    """add() stage + 3 times from ptr 7: the full stage ships on its own (past capacity where
    cap < stage), the last three rows with the flush that reading ptr makes."""
    rec = _rec(shape)
    rb, model = _ring(shape, cap)
    assert len(rb._stage) == stage
    rs = np.random.RandomState(5)
    _add_batch(rb, model, shape, _rows(rs, shape, 7))
    rows = _rows(rs, shape, stage + 3)
    assert _route(stage, cap, rec) == {(17, 6): "put", (3, 1): "put", (7, 16, 9, 3): "memcpy",
                                       (3, 5, 3, 2): "put"}[shape]
    assert _route(3, cap, rec) == "args"
    for i in range(stage):
        _add_one(rb, model, shape, rows, i)
    assert rb._n == 0                                         # the automatic flush ran
    for i in range(stage, stage + 3):
        _add_one(rb, model, shape, rows, i)
    assert rb._n == 3
    _same(rb, model)
    assert (model.ptr, model.size) == ((7 + stage + 3) % cap, min(7 + stage + 3, cap))
