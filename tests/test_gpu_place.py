"""GPU: the place-recognition entry points (include/loamx.h, "place recognition") against the numpy model of tests/place_common.py,
by equality of bytes: descriptors, ring keys, column norms and the records of a search. The model reads the database's own sector
table (loamx_place_db_sector_dirs) and asserts that every valid point has exactly one sector."""
import ctypes as C

import numpy as np
import pytest

import outdoor_scenes as S
import place_common as M
from gpu_common import ctx
from loam_amd import capi

pytestmark = pytest.mark.gpu


def make_db(R, S_, **kw):
    return ctx().place_db(capi.PlaceParams(n_rings=R, n_sectors=S_, **kw))


def model_desc(db, pts):
    p = db.params
    return M.descriptor(pts, db.sector_dirs(), p.n_rings, p.max_range, p.z_offset, p.z_scale)


def same_desc(got, want, where):
    assert got.dtype == np.uint16 and got.shape == want.shape, (where, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), (where, len(bad), bad[:5].tolist(), got[got != want][:5].tolist(), want[got != want][:5].tolist())


def run_desc_dev(db, clouds, poison=0xA5):
    """loamx_place_descriptors_dev[_f32] on a poisoned output -> (n_clouds, R, S) uint16"""
    c = ctx()
    dt = clouds[0].dtype
    off = np.concatenate([[0], np.cumsum([len(a) for a in clouds])]).astype(np.uint64)
    pts = np.ascontiguousarray(np.concatenate(clouds, axis=0))
    nc = len(clouds)
    d_pts, d_desc = c.alloc(max(pts.nbytes, 8)), c.alloc(nc * db.cells * 2)
    try:
        if len(pts):
            d_pts.upload(pts)
        d_desc.upload(np.full(d_desc.nbytes, poison, dtype=np.uint8))
        db.descriptors_dev(d_pts.ptr, clouds[0].shape[1], off, d_desc.ptr, f32=dt == np.float32)
        c.synchronize()
        return d_desc.download(np.uint16, nc * db.cells).reshape(nc, db.n_rings, db.n_sectors)
    finally:
        d_pts.free(), d_desc.free()


def run_search_dev(db, queries, K, id_end=None, poison=0xA5):
    """loamx_place_search_dev on a poisoned output -> (n, K) records"""
    c = ctx()
    q = np.ascontiguousarray(queries, dtype=np.uint16).reshape(-1, db.n_rings, db.n_sectors)
    d_q, d_out = c.alloc(q.nbytes), c.alloc(len(q) * K * capi.PLACE_MATCH_DTYPE.itemsize)
    try:
        d_q.upload(q)
        d_out.upload(np.full(d_out.nbytes, poison, dtype=np.uint8))
        db.search_dev(d_q.ptr, len(q), K, d_out.ptr, id_end=id_end)
        c.synchronize()
        return d_out.download(capi.PLACE_MATCH_DTYPE, len(q) * K).reshape(len(q), K)
    finally:
        d_q.free(), d_out.free()


def model_search(queries, entries, K, id_end=None):
    n = len(queries)
    ends = [None] * n if id_end is None else np.broadcast_to(np.asarray(id_end), (n,))
    return np.stack([M.search(q, entries, K, e) for q, e in zip(queries, ends)])


def test_the_record_layout_is_the_c_struct():
    assert capi.PLACE_MATCH_DTYPE.itemsize == 24 and capi.PLACE_MATCH_DTYPE == M.MATCH_DTYPE
    assert [capi.PLACE_MATCH_DTYPE.fields[n][1] for n in ("id", "shift", "key_dist", "distance")] == [0, 4, 8, 16]


def test_cloud_sizes_around_the_wavefront_and_the_workgroup():
    db = make_db(3, 5, max_range=60.0)
    rng = np.random.default_rng(71)
    try:
        for n in (0, 1, 63, 64, 65, 255, 256, 257, 1025):
            pts = M.random_cloud(rng, n)
            same_desc(db.descriptor(pts), model_desc(db, pts), "n = %d" % n)
        assert (db.descriptor(M.random_cloud(rng, 1025)) != 0).sum() >= 12
    finally:
        db.close()


@pytest.mark.parametrize("R,S_,n", [(1, 3, 300), (3, 5, 20000), (20, 60, 20000), (64, 360, 30000)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_shapes_and_clouds_that_several_workgroups_share(R, S_, n, dtype):
    """(20 000 points are several workgroups' worth at any launch the build could sensibly make; 64 x 360 is the shape whose
    table does not fit the LDS)"""
    db = make_db(R, S_)
    pts = M.random_cloud(np.random.default_rng([72, R, S_]), n).astype(dtype)
    try:
        got = db.descriptor(pts)
        same_desc(got, model_desc(db, pts), "%d x %d" % (R, S_))
        assert (got != 0).sum() > min(R * S_, n) // 4
    finally:
        db.close()


def test_point_stride_4_and_the_edges_of_the_rule():
    db = make_db(3, 5, max_range=60.0)
    rng = np.random.default_rng(73)
    pts = np.concatenate([M.random_cloud(rng, 500), rng.uniform(-1, 1, (500, 1))], axis=1)
    edge = np.array([[20.0, 0, 0], [np.nextafter(20.0, 0), 0, 0], [np.nextafter(20.0, 99), 0, 0], [60.0, 0, 0], [np.nextafter(60.0, 0), 0, 0],
                     [0, 0, 5.0], [1e-50, 0, 1.0], [1e-51, 1e-51, 1.0], [np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [1e200, 1, 1],
                     [5, 5, -2.0], [5, -5, np.nextafter(-2.0, -9)], [-5, 5, 1021.984375], [-5, -5, 1021.96875], [7, 1, 1e150], [7, -1, -1e150]])
    pts = np.concatenate([pts, np.concatenate([edge, np.zeros((len(edge), 1))], axis=1)])
    try:
        same_desc(db.descriptor(pts), model_desc(db, pts), "stride 4")
        same_desc(db.descriptor(pts.astype(np.float32)), model_desc(db, pts.astype(np.float32)), "stride 4, float")
        same_desc(run_desc_dev(db, [pts])[0], model_desc(db, pts), "stride 4, device form")
    finally:
        db.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_batch_equals_its_clouds_one_by_one_and_two_runs_give_the_same_bytes(dtype):
    db = make_db(20, 60)
    rng = np.random.default_rng(74)
    clouds = [M.random_cloud(rng, n).astype(dtype) for n in (5000, 0, 64, 300, 2049)]
    try:
        first = run_desc_dev(db, clouds, poison=0xA5)
        again = run_desc_dev(db, clouds, poison=0x3C)
        assert first.tobytes() == again.tobytes()
        assert not first[1].any()
        for i, cl in enumerate(clouds):
            same_desc(first[i], model_desc(db, cl), "cloud %d of the batch" % i)
            same_desc(run_desc_dev(db, [cl])[0], first[i], "cloud %d alone" % i)
            same_desc(db.descriptor(cl), first[i], "cloud %d, host form" % i)
    finally:
        db.close()


def test_a_batch_of_more_clouds_than_one_launch_takes():
    db = make_db(3, 5, max_range=60.0)
    rng = np.random.default_rng(75)
    clouds = [M.random_cloud(rng, int(n)) for n in rng.integers(0, 40, 300)]
    try:
        got = run_desc_dev(db, clouds)
        for i in (0, 1, 255, 256, 257, 299):
            same_desc(got[i], model_desc(db, clouds[i]), "cloud %d" % i)
    finally:
        db.close()


def test_entries_added_in_several_calls_across_a_growth_equal_one_add():
    rng = np.random.default_rng(76)
    d = M.random_descriptors(rng, 700, 4, 6, hi=65536)
    d[5] = 65535
    d[6] = 0
    a, b = make_db(4, 6), make_db(4, 6)
    try:
        assert a.size() == 0
        firsts = [a.add(d[:3]), a.add(d[3:3]), a.add(d[3:250]), a.add(d[250:257]), a.add(d[257:])]
        assert firsts == [0, 3, 3, 250, 257] and a.size() == 700
        assert b.add(d) == 0 and b.size() == 700
        for db in (a, b):
            desc, keys, norms = db.read()
            assert desc.tobytes() == d.tobytes()
            assert keys.dtype == np.uint32 and keys.tobytes() == M.ring_keys(d).tobytes()
            assert norms.dtype == np.uint64 and norms.tobytes() == M.column_norms(d).tobytes()
        desc, keys, norms = a.read(255, 3)
        assert desc.tobytes() == d[255:258].tobytes() and keys.tobytes() == M.ring_keys(d[255:258]).tobytes()
    finally:
        a.close(), b.close()


def test_keys_and_norms_at_their_largest_values():
    d = np.full((2, 64, 360), 65535, dtype=np.uint16)
    db = make_db(64, 360)
    try:
        db.add(d)
        desc, keys, norms = db.read()
        assert (keys == 65535 * 360).all() and (norms == 64 * 65535 ** 2).all()
        got = db.search(d[0], 2)
        M.same_records(got[0], M.search(d[0], d, 2), "all codes 65535")
        assert got[0]["distance"].tolist() == [0.0, 0.0] and got[0]["id"].tolist() == [0, 1]
    finally:
        db.close()


@pytest.mark.parametrize("K", [1, 5, 64])
def test_search_at_database_sizes_around_k_and_the_chunk(K):
    rng = np.random.default_rng([77, K])
    sizes = sorted({0, K - 1, K, K + 1, 63, 64, 65, 257, 1025})
    d = M.random_descriptors(rng, 1025, 4, 6)
    d[40], d[900] = d[7], d[7]  # (duplicates: key and distance ties)
    queries = np.concatenate([d[[7, 63, 1024]], M.random_descriptors(rng, 2, 4, 6)])
    db = make_db(4, 6)
    try:
        have = 0
        for n in sizes:
            if n > have:
                db.add(d[have:n])
                have = n
            got = run_search_dev(db, queries, K)
            M.same_records(got, model_search(queries, d[:n], K).astype(capi.PLACE_MATCH_DTYPE), "N = %d" % n)
            if n >= 1025 and K >= 5:
                assert got[0]["id"][:3].tolist() == [7, 40, 900] and not got[0]["distance"][:3].any()
    finally:
        db.close()


def test_search_over_several_chunks_and_merge_passes():
    """3000 entries are three chunks of the first pass; at K = 64 their 192 records take a second pass"""
    rng = np.random.default_rng(78)
    d = M.random_descriptors(rng, 3000, 4, 6)
    d[2999], d[1024], d[5] = d[1500], d[1500], d[1500]
    queries = np.concatenate([d[[1500, 0]], M.random_descriptors(rng, 2, 4, 6)])
    db = make_db(4, 6)
    try:
        db.add(d)
        for K in (3, 64):
            got = run_search_dev(db, queries, K)
            M.same_records(got, model_search(queries, d, K).astype(capi.PLACE_MATCH_DTYPE), "K = %d" % K)
        assert got[0]["id"][:4].tolist() == [5, 1024, 1500, 2999]
        ends = [3000, 1500, 1025, 0]
        M.same_records(run_search_dev(db, queries, 5, id_end=ends), model_search(queries, d, 5, ends).astype(capi.PLACE_MATCH_DTYPE), "id_end")
    finally:
        db.close()


@pytest.mark.parametrize("R,S_", [(4, 6), (20, 60)])
def test_a_rolled_descriptor_is_found_with_its_shift_and_distance_zero(R, S_):
    rng = np.random.default_rng([79, S_])
    d = M.random_descriptors(rng, 5, R, S_)
    d[2, :, 0] = np.maximum(d[2, :, 0], 1)  # (entry 2: no two shifts alike)
    db = make_db(R, S_)
    try:
        db.add(d)
        queries = np.stack([np.roll(d[2], -s, axis=1) for s in range(S_)])
        got = db.search(queries, 5)
        assert got[:, 0]["id"].tolist() == [2] * S_
        assert got[:, 0]["shift"].tolist() == list(range(S_))
        assert got[:, 0]["distance"].tolist() == [0.0] * S_ and got[:, 0]["key_dist"].tolist() == [0] * S_
        M.same_records(got[::7], model_search(queries[::7], d, 5).astype(capi.PLACE_MATCH_DTYPE), "rolled")
    finally:
        db.close()


def test_ties_a_periodic_descriptor_and_an_all_zero_query():
    rng = np.random.default_rng(80)
    base = M.random_descriptors(rng, 1, 4, 2, fill=1.0)[0]
    periodic = np.tile(base, (1, 3))  # (S = 6 with period 2: the shifts 0, 2, 4 tie)
    d = np.stack([periodic, M.random_descriptors(rng, 1, 4, 6)[0], periodic, np.zeros((4, 6), np.uint16)])
    db = make_db(4, 6)
    try:
        db.add(d)
        got = db.search(np.stack([np.roll(periodic, -1, axis=1), np.zeros((4, 6), np.uint16)]), 4)
        M.same_records(got, model_search([np.roll(periodic, -1, axis=1), np.zeros((4, 6), np.uint16)], d, 4).astype(capi.PLACE_MATCH_DTYPE), "ties")
        assert got[0]["id"][:2].tolist() == [0, 2] and got[0]["shift"][:2].tolist() == [1, 1] and not got[0]["distance"][:2].any()
        assert got[1]["distance"].tolist() == [1.0] * 4 and got[1]["shift"].tolist() == [0] * 4
        assert got[1]["id"].tolist() == [0, 1, 2, 3]  # (equal distances: by id)
    finally:
        db.close()


def test_id_end_per_query_a_batch_against_single_queries_and_the_host_form():
    rng = np.random.default_rng(81)
    d = M.random_descriptors(rng, 300, 20, 60)
    queries = np.concatenate([d[[10, 10, 200, 200, 299]], M.random_descriptors(rng, 1, 20, 60)])
    ends = [0, 1, 200, 201, 300, 5000]
    db = make_db(20, 60)
    try:
        db.add(d)
        batch = run_search_dev(db, queries, 4, id_end=ends, poison=0xA5)
        assert batch.tobytes() == run_search_dev(db, queries, 4, id_end=ends, poison=0x3C).tobytes()
        M.same_records(batch, model_search(queries, d, 4, ends).astype(capi.PLACE_MATCH_DTYPE), "batch")
        assert batch[0]["id"].tolist() == [capi.PLACE_NO_ID] * 4 and batch[0]["distance"].tolist() == [2.0] * 4
        assert batch[0]["key_dist"].tolist() == [2 ** 64 - 1] * 4 and batch[0]["shift"].tolist() == [0] * 4
        assert batch[1]["id"].tolist() == [0] + [capi.PLACE_NO_ID] * 3
        assert batch[3]["id"][0] == 200 and batch[3]["distance"][0] == 0.0 and batch[2]["id"][0] != 200 and batch[4]["id"][0] == 299
        for i in range(len(queries)):
            M.same_records(run_search_dev(db, queries[i], 4, id_end=ends[i])[0], batch[i], "query %d alone" % i)
        M.same_records(db.search(queries, 4, id_end=ends), batch, "host form")
        M.same_records(db.search(queries, 4), run_search_dev(db, queries, 4), "host form, every entry")
        M.same_records(db.search(queries, 4, id_end=300), db.search(queries, 4), "one id_end for all")
    finally:
        db.close()


def test_more_queries_with_an_id_end_than_one_launch_carries():
    rng = np.random.default_rng(82)
    d = M.random_descriptors(rng, 40, 4, 6)
    queries = M.random_descriptors(rng, 300, 4, 6)
    ends = rng.integers(0, 45, 300)
    db = make_db(4, 6)
    try:
        db.add(d)
        got = run_search_dev(db, queries, 2, id_end=ends)
        pick = [0, 255, 256, 257, 299]
        M.same_records(got[pick], model_search(queries[pick], d, 2, ends[pick]).astype(capi.PLACE_MATCH_DTYPE), "query groups")
    finally:
        db.close()


def test_refusals_leave_the_database_as_it_was():
    c, lib = ctx(), capi.load()
    for bad, status in ((dict(n_rings=0), capi.ERR_BAD_PARAM), (dict(n_sectors=0), capi.ERR_BAD_PARAM),
                        (dict(max_range=0.0), capi.ERR_BAD_PARAM), (dict(max_range=-1.0), capi.ERR_BAD_PARAM),
                        (dict(max_range=np.inf), capi.ERR_BAD_PARAM), (dict(max_range=np.nan), capi.ERR_BAD_PARAM),
                        (dict(z_scale=0.0), capi.ERR_BAD_PARAM), (dict(z_scale=np.inf), capi.ERR_BAD_PARAM), (dict(z_scale=np.nan), capi.ERR_BAD_PARAM),
                        (dict(z_offset=np.nan), capi.ERR_BAD_PARAM), (dict(z_offset=np.inf), capi.ERR_BAD_PARAM),
                        (dict(n_rings=65), capi.ERR_UNSUPPORTED), (dict(n_sectors=2), capi.ERR_UNSUPPORTED), (dict(n_sectors=361), capi.ERR_UNSUPPORTED)):
        with pytest.raises(capi.LoamxError) as e:
            c.place_db(capi.PlaceParams(**bad))
        assert e.value.status == status, bad
    h = C.c_void_p()
    assert lib.loamx_place_db_create(c.h, None, C.byref(h)) == capi.ERR_BAD_PARAM
    st = capi.PlaceParams().struct()
    assert lib.loamx_place_db_create(c.h, C.byref(st), None) == capi.ERR_BAD_PARAM
    assert lib.loamx_place_db_sector_dirs(None, None) == capi.ERR_BAD_PARAM and lib.loamx_place_db_size(None, None) == capi.ERR_BAD_PARAM

    rng = np.random.default_rng(83)
    d = M.random_descriptors(rng, 10, 4, 6)
    db = make_db(4, 6)
    d_q, d_out, d_pts = c.alloc(d.nbytes), c.alloc(10 * 64 * 24), c.alloc(24 * 16)
    off = (C.c_size_t * 2)(0, 16)
    down = (C.c_size_t * 3)(0, 16, 8)
    try:
        db.add(d)
        d_q.upload(d)
        d_out.upload(np.full(d_out.nbytes, 0x5A, dtype=np.uint8))
        before = [a.tobytes() for a in db.read()]
        calls = [
            (lib.loamx_place_search_dev(c.h, db.h, d_q.ptr, 10, None, 0, d_out.ptr), capi.ERR_BAD_PARAM),
            (lib.loamx_place_search_dev(c.h, db.h, d_q.ptr, 10, None, 65, d_out.ptr), capi.ERR_BAD_PARAM),
            (lib.loamx_place_search_dev(c.h, None, d_q.ptr, 10, None, 3, d_out.ptr), capi.ERR_BAD_PARAM),
            (lib.loamx_place_search_dev(c.h, db.h, None, 10, None, 3, d_out.ptr), capi.ERR_BAD_PARAM),
            (lib.loamx_place_search_dev(c.h, db.h, d_q.ptr, 10, None, 3, None), capi.ERR_BAD_PARAM),
            (lib.loamx_place_db_add_dev(c.h, db.h, None, 3, None), capi.ERR_BAD_PARAM),
            (lib.loamx_place_db_add_dev(c.h, None, d_q.ptr, 3, None), capi.ERR_BAD_PARAM),
            (lib.loamx_place_db_add_dev(c.h, db.h, d_q.ptr, (1 << 24) - 9, None), capi.ERR_UNSUPPORTED),
            (lib.loamx_place_db_add_dev(c.h, db.h, d_q.ptr, (1 << 24) + 1, None), capi.ERR_UNSUPPORTED),
            (lib.loamx_place_db_read(c.h, db.h, 5, 6, None, None, None), capi.ERR_BAD_PARAM),
            (lib.loamx_place_db_read(c.h, db.h, 11, 0, None, None, None), capi.ERR_BAD_PARAM),
            (lib.loamx_place_descriptors_dev(c.h, db.h, d_pts.ptr, 2, off, 1, d_out.ptr), capi.ERR_BAD_PARAM),
            (lib.loamx_place_descriptors_dev(c.h, db.h, None, 3, off, 1, d_out.ptr), capi.ERR_BAD_PARAM),
            (lib.loamx_place_descriptors_dev(c.h, db.h, d_pts.ptr, 3, None, 1, d_out.ptr), capi.ERR_BAD_PARAM),
            (lib.loamx_place_descriptors_dev(c.h, db.h, d_pts.ptr, 3, off, 1, None), capi.ERR_BAD_PARAM),
            (lib.loamx_place_descriptors_dev(c.h, None, d_pts.ptr, 3, off, 1, d_out.ptr), capi.ERR_BAD_PARAM),
            (lib.loamx_place_descriptors_dev_f32(c.h, db.h, d_pts.ptr, 3, down, 2, d_out.ptr), capi.ERR_BAD_PARAM),
        ]
        for i, (rc, want) in enumerate(calls):
            assert rc == want, (i, rc, want)
        # the calls that have nothing to do
        assert lib.loamx_place_search_dev(c.h, db.h, None, 0, None, 3, None) == capi.OK
        assert lib.loamx_place_descriptors_dev(c.h, db.h, None, 3, None, 0, None) == capi.OK
        assert lib.loamx_place_db_add_dev(c.h, db.h, None, 0, None) == capi.OK
        c.synchronize()
        assert db.size() == 10 and [a.tobytes() for a in db.read()] == before
        assert (d_out.download(np.uint8, d_out.nbytes) == 0x5A).all()  # (a refused call writes nothing)
        M.same_records(db.search(d[:2], 3), model_search(d[:2], d, 3).astype(capi.PLACE_MATCH_DTYPE), "after the refusals")
    finally:
        d_q.free(), d_out.free(), d_pts.free()
        db.close()


def test_places_are_recognised_with_their_shift():
    """12 places (canyon, lot and field, scene seeds 0 .. 3) at H x W = 16 x 256; query i is cast from the same place moved by
    (0.4, -0.2, 0) in its own frame and turned by k_i sectors, k_i = (7 i + 3) mod 60. With K = 3 every query's first record is
    its own place with shift k_i (the ordering and the shift, not the distance values)."""
    H, W = 16, 256
    places = [(name, seed) for name in S.SCENES for seed in range(4)]
    entries, queries = [], []
    for i, (name, seed) in enumerate(places):
        o, yaw = S.sensor_origin(name, seed)
        entries.append(S.scan_at(name, seed, o, yaw, H, W, noise_seed=1))
        k = (7 * i + 3) % 60
        o_q = o + S._rz(yaw) @ np.array([0.4, -0.2, 0.0])
        queries.append(S.scan_at(name, seed, o_q, yaw + k * 2.0 * np.pi / 60, H, W, noise_seed=100 + i))
    db = ctx().place_db()
    try:
        got = run_desc_dev(db, entries + queries)
        for i in (0, 5, 11, 12, 23):
            same_desc(got[i], model_desc(db, (entries + queries)[i]), "scan %d" % i)
        db.add(got[:12])
        rec = db.search(got[12:], 3)
        M.same_records(rec, model_search(got[12:], got[:12], 3).astype(capi.PLACE_MATCH_DTYPE), "places")
        assert rec[:, 0]["id"].tolist() == list(range(12))
        assert rec[:, 0]["shift"].tolist() == [(7 * i + 3) % 60 for i in range(12)]
        assert (rec[:, 0]["distance"] < rec[:, 1]["distance"]).all()
    finally:
        db.close()
