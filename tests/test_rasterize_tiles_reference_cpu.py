"""The case table of tests/test_rasterize_tiles_gpu.py reaches every path of the tiled rasteriser: checked on the restatement of the
kernel's decisions (``rasterize_forms``), without a device."""
import rasterize_tiles_cases as T


def test_tile_table_reaches_every_path():
    seen, passes = T.coverage()
    print(seen, sorted(passes))
    for key in ('none', 'one', 'two', 'direct'):
        assert seen[key] >= 8, (key, seen)
    # a tile whose waves take different paths: the direct form beside a merged one, one window beside two
    for key in ('tile direct + merged', 'tile one + two', 'crop tabulated', 'crop looped', 'tile crop tabulated + looped'):
        assert seen[key] > 0, (key, seen)
    # channel passes of 64 lanes: a partly filled single pass, a second pass, five passes with a ragged end, for 4 channels and 1 channel a lane
    assert {(4, 1), (4, 2), (4, 5), (1, 5)} <= passes
    assert {c.res for c in T.CASES} == {64, 128} and {c.B for c in T.CASES} == {1, 2}
    assert {6, 36, 260, 1032} <= {c.C for c in T.CASES}
