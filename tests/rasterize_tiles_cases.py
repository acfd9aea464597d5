"""Case table of the tiled rasteriser (rasterize_tile_kernel of csrc/rasterize.hip: a workgroup of four waves owns 16 x 1 output pixels,
i.e. four 4-pixel groups, one per wave), over the inputs and the restatements of tests/frame_glue_reference.py.  No device code.

The launcher accepts res = 32, 64, 128 only (tests/test_frame_glue_gpu.py asserts that it refuses the others), and the tile divides all
three, so a partial tile cannot be reached through the entry point; the 32^2 level keeps the one-group kernel.  The cases are therefore
at 64 and 128: channel counts below, at and above one pass of 64 lanes x 4 channels (6 and 36: one partly filled pass; 260: a second
pass with one lane; 1032: five passes, the last ragged; 261: one channel per lane, five passes), two images (tile -> (b, y, x) and the
XCD bands cross the image boundary), the three kinds of UV map, and a static crop whose window exceeds the 3 x 6 table in some groups."""
import frame_glue_reference as R

TILE_GROUPS = 4          # groups of a tile, side by side in x

CASES = (
    R.Rast('tile smooth 128, C = 6', 'face', 128, 6, B=2),
    R.Rast('tile smooth 64, C = 260', 'face', 64, 260, B=2),
    R.Rast('tile silhouette 128, C = 36', 'silhouette', 128, 36, B=2),
    R.Rast('tile silhouette 64, C = 1032', 'silhouette', 64, 1032),
    R.Rast('tile seam 128, C = 36', 'seam:-0.9,-0.7,-0.5', 128, 36, B=2),
    R.Rast('tile seam 64, C = 261', 'seam', 64, 261),
    R.Rast('tile seam 64, C = 6', 'seam:-0.9,-0.7,-0.5', 64, 6, B=2),
    R.Rast('tile padding 64, C = 6', 'padding', 64, 6),
    R.Rast('tile crop 40 x 84 at 64', 'silhouette', 64, 36, B=2, crop=(3, 43, 5, 89), sta_res=100),     # 6 or 7 columns a group: table | loop
    R.Rast('tile crop 100 at 64', 'face', 64, 6, crop=(0, 100, 0, 100), sta_res=100),
)

DETERMINISM_CASE = CASES[4]


def tile_forms(case):
    """forms [B, res, res / 16, 4]: the form (R.FORMS) of the four groups of every tile."""
    f = R.rast_forms(case)['form']
    return f.reshape(case.B, case.res, case.res // (4 * TILE_GROUPS), TILE_GROUPS)


def coverage(cases=CASES):
    """What the table reaches: groups per form, tiles that mix the direct form with a merged one, tiles that mix one and two windows,
    groups with a tabulated and with a looped crop, channel passes."""
    seen = {'none': 0, 'one': 0, 'two': 0, 'direct': 0, 'tile direct + merged': 0, 'tile one + two': 0, 'crop tabulated': 0, 'crop looped': 0,
            'tile crop tabulated + looped': 0}
    passes = set()
    for case in cases:
        f = R.rast_forms(case)
        t = tile_forms(case)
        for k, name in enumerate(R.FORMS):
            seen[name] += int((t == k).sum())
        seen['tile direct + merged'] += int(((t == 3).any(-1) & (t < 3).any(-1)).sum())
        seen['tile one + two'] += int(((t == 1).any(-1) & (t == 2).any(-1)).sum())
        tab = f['crop_tabulated'].reshape(case.res, case.res // (4 * TILE_GROUPS), TILE_GROUPS)
        seen['crop tabulated'] += int(tab.sum())
        seen['crop looped'] += int((~tab).sum())
        seen['tile crop tabulated + looped'] += int((tab.any(-1) & ~tab.all(-1)).sum())
        cv = 4 if case.C % 4 == 0 else 1
        ncq = -(-case.C // cv)
        passes.add((cv, -(-ncq // 64)))
    return seen, passes
