"""The batch ingest's route table and slot layout (mlhot/ingest.py ROUTES, slot_layout, check_table): plain integers, no GPU and no
library.  The expected offsets are written out here from the layout's definition, never taken from slot_layout:

    byte route: [ctx images | qry images | pad16 | ctx labels | qry labels]
    id route:   [ids int32 | bg int32 (RGBA pool only) | pad16 | ctx labels | qry labels]
    with a table, both append [pad16 | records int32 [n, ints] | LUTs uint8 [n, 256]]; the buffer is at least 16 bytes."""
import numpy as np
import pytest

from mlhot import augment as A
from mlhot.binding import MlhotError
from mlhot.ingest import BYTES, GREY, RGBA, ROUTES, check_table, slot_layout

TABLES = {None: 0, A.AugTable: 32, A.ImageAugTable: 40}              # table kind -> int32s per record
ROWS = [(source, table) for source in (BYTES, RGBA, GREY) for table in TABLES if (source, table) != (RGBA, A.AugTable)]
# (T, Nc, Nq, ctx H x W, qry H x W): the shared geometry, ctx 8 x 8 against qry 12 x 8 (byte routes only), and an empty context
CASES = [(2, 3, 2, (8, 8), (8, 8)), (2, 3, 2, (8, 8), (12, 8)), (2, 0, 2, (8, 8), (8, 8))]
LAYOUTS = [row + case for row in ROWS for case in CASES if row[0] == BYTES or case[3] == case[4]]       # ids carry no geometry


def pad16(n):
    return (n + 15) // 16 * 16


def test_the_table_has_the_eight_legal_rows():
    assert len(ROUTES) == 8 and set(ROUTES) == set(ROWS)
    assert len({r.name for r in ROUTES.values()}) == 8                               # the name ends the slot key: one ring per route
    for (source, table), r in ROUTES.items():
        assert (r.source, r.table, r.record_ints) == (source, table, TABLES[table])
        assert r.ids == (source != BYTES) and r.bg == (source == RGBA)
        assert r.channels == {BYTES: 0, RGBA: 3, GREY: 1}[source]
    assert [ROUTES[k].name for k in ROWS if k[0] != BYTES] == ["pool", "poolaug", "pool1", "pool1aug", "pool1augimg"]
    assert [ROUTES[k].entry for k in ROWS] == ["ingest_u8_nhwc", "augment_ingest_u8", "augment_ingest_u8_img", "pool_ingest_u8",
                                               "pool_augment_ingest_u8_img", "pool1_ingest_u8", "pool1_augment_ingest_u8",
                                               "pool1_augment_ingest_u8_img"]


@pytest.mark.parametrize("source,table,T,Nc,Nq,g0,g1", LAYOUTS, ids=lambda v: getattr(v, "__name__", None))
def test_slot_layout_is_the_written_out_layout(source, table, T, Nc, Nq, g0, g1):
    route = ROUTES[source, table]
    C = 1 if table is A.AugTable or source == GREY else 3
    lab = ((T, Nc, 3), (T, Nq, 3))
    key = (((T, Nc), (T, Nq)) if route.ids else ((T, Nc, *g0, C), (T, Nq, *g1, C))) + lab
    n = T * Nc + T * Nq
    if source == BYTES:
        parts = (0, T * Nc * g0[0] * g0[1] * C, T * Nc * g0[0] * g0[1] * C + T * Nq * g1[0] * g1[1] * C)
    else:
        parts = (0, 4 * n, 8 * n) if source == RGBA else (0, 4 * n)
    lab_off = pad16(parts[-1])
    lab_mid = lab_off + 4 * T * Nc * 3
    lab_end = lab_mid + 4 * T * Nq * 3
    rec_off = pad16(lab_end)
    lut_off = rec_off + 4 * TABLES[table] * n
    end = lab_end if table is None else lut_off + 256 * n

    lay = slot_layout(route, key)
    assert lay.parts == parts and lay.n_img == n
    assert (lay.lab_off, lay.lab_mid, lay.lab_end, lay.rec_off, lay.lut_off) == (lab_off, lab_mid, lab_end, rec_off, lut_off)
    assert lay.total == max(end, 16) and lay.total >= 16
    assert lay.lab_off % 16 == 0 and lay.rec_off % 16 == 0 and lay.lut_off % 16 == 0
    # the sections are disjoint and in order, and the last one in use ends inside the buffer
    bounds = [*lay.parts, lay.lab_off, lay.lab_mid, lay.lab_end] + ([lay.rec_off, lay.lut_off, lay.lut_off + 256 * n] if table else [])
    assert bounds == sorted(bounds) and bounds[0] == 0 and bounds[-1] <= lay.total


def _table(kind, n, ints=None, spec="shapenet_3d"):
    records = np.zeros((n, TABLES[kind] if ints is None else ints), dtype=np.int32)
    luts = np.zeros((0, 256), dtype=np.uint8)
    return A.AugTable(records, luts) if kind is A.AugTable else A.ImageAugTable(records, luts, A.ImageAugmentSpec.for_task(spec))


def test_check_table_returns_the_route_or_refuses():
    for source, table in ROWS:
        t = None if table is None else _table(table, 10)
        assert check_table(source, t, 10) is ROUTES[source, table]
    with pytest.raises(MlhotError, match="RGBA pool.*got AugTable"):
        check_table(RGBA, _table(A.AugTable, 10), 10)                                # not a row
    with pytest.raises(MlhotError, match="pre_op"):
        check_table(RGBA, _table(A.ImageAugTable, 10, spec="distractor"), 10)        # (pre_op, div2) = (1, 255): Distractor's bytes
    for source in (BYTES, RGBA, GREY):
        with pytest.raises(MlhotError, match="got ndarray"):
            check_table(source, np.zeros((10, 40), dtype=np.int32), 10)              # wrong type: bare records
        with pytest.raises(MlhotError, match=r"\[n, 40\]"):
            check_table(source, _table(A.ImageAugTable, 10, ints=32), 10)            # wrong record width
        with pytest.raises(MlhotError, match="10 records for 9 images"):
            check_table(source, _table(A.ImageAugTable, 10), 9)                      # wrong record count
    with pytest.raises(MlhotError, match=r"\[n, 32\]"):
        check_table(GREY, _table(A.AugTable, 10, ints=40), 10)
    assert check_table(BYTES, _table(A.AugTable, 10), 10, channels=(1, 1)).name == "aug"
    for channels in ((3, 3), (1, 3), (3, 1)):
        with pytest.raises(MlhotError, match="single-channel"):
            check_table(BYTES, _table(A.AugTable, 10), 10, channels=channels)        # the 1D sequences on multi-channel images
    assert check_table(BYTES, _table(A.ImageAugTable, 10), 10, channels=(3, 3)).name == "augimg"
    with pytest.raises(MlhotError, match="bg must be None"):
        check_table(GREY, None, 10, bg=np.full(10, -1))                              # bg on a grey pool
    assert check_table(RGBA, None, 10, bg=np.full(10, -1)).name == "pool"
