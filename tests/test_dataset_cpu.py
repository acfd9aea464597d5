"""`training_avatar_texture.dataset_new.ImageFolderDataset` (the scripts' reader of the on-disk format, eval_seq.py:106-128,204):
known answers on a dataset written by this test, and item-by-item equality with what the reference's class returns for the same
directory (stored under tests/golden/)."""
import json
import os

import numpy as np
import PIL.Image
import pytest

from invertavatar_amd.training_avatar_texture import dataset_new


def _write_dataset(root, videos=('vidA', 'vidB'), frames=3, res=16, uv_res=8, rgba=False):
    rs = np.random.RandomState(5)
    img_root = root / 'dataset' / 'images512x512'
    names, cams, labels = [], [], []
    for v in videos:
        for k in range(frames):
            name = f'{v}/{k * 30:08d}.png'
            names.append(name)
            for folder in ('images512x512', 'fgmasks512x512', 'uvRender256x256', 'orthRender256x256_face_eye', 'coeffs'):
                (root / 'dataset' / folder / v).mkdir(parents=True, exist_ok=True)
            ch = 4 if rgba else 3
            PIL.Image.fromarray(rs.randint(0, 256, (res, res, ch)).astype(np.uint8)).save(img_root / name)
            PIL.Image.fromarray(rs.randint(0, 256, (res, res)).astype(np.uint8)).save(root / 'dataset' / 'fgmasks512x512' / name)
            stem = name.split('.')[0]
            np.save(root / 'dataset' / 'uvRender256x256' / (stem + '.npy'), rs.randn(uv_res, uv_res, 4).astype(np.float16))
            PIL.Image.fromarray(rs.randint(0, 256, (uv_res, uv_res, 3)).astype(np.uint8)).save(
                root / 'dataset' / 'uvRender256x256' / (stem + '_uvgttex.png'))
            np.save(root / 'dataset' / 'orthRender256x256_face_eye' / (stem + '.npy'), rs.rand(uv_res, uv_res, 4).astype(np.float32))
            np.save(root / 'dataset' / 'coeffs' / (stem + '.npy'), rs.randn(20).astype(np.float64))
            cams.append([name, rs.randn(25).tolist()])
            labels.append([name, rs.randn(25).tolist()])
    (img_root / 'dataset_realcam.json').write_text(json.dumps({'labels': cams}))
    (img_root / 'dataset.json').write_text(json.dumps({'labels': labels[::-1]}))       # order of the label file must not matter
    mask_dir = root / 'data_preprocess' / 'FaceVerse' / 'v3'
    mask_dir.mkdir(parents=True)
    PIL.Image.fromarray((rs.rand(uv_res, uv_res) > 0.4).astype(np.uint8) * 255).save(mask_dir / 'dense_uv_expanded_mask_onlyFace.png')
    return str(img_root), names, dict(cams), dict(labels)


def _kwargs(path, **extra):
    base = os.path.dirname(path)
    return dict(path=path, mesh_path=os.path.join(base, 'orthRender256x256_face_eye'), label_file='dataset.json',
                fvcoeffs_path=os.path.join(base, 'coeffs'), return_name=True, **extra)


def test_known_answers(tmp_path, monkeypatch):
    path, names, cams, labels = _write_dataset(tmp_path)
    monkeypatch.chdir(tmp_path)               # the UV face mask is read relative to the working directory (dataset_new.py:228)
    ds = dataset_new.ImageFolderDataset(**_kwargs(path, load_uv=True, load_bg=True))
    assert len(ds) == 6 and ds.name == 'images512x512' and ds.label_shape == [25] and ds.label_dim == 25 and ds.has_labels
    name, image, label_cam, vert = ds[4]
    assert name == names[4]
    rgb = np.asarray(PIL.Image.open(os.path.join(path, name))).transpose(2, 0, 1)
    assert image['image'].shape == (4, 16, 16) and image['image'].dtype == np.uint8 and np.array_equal(image['image'][:3], rgb)
    mask = np.asarray(PIL.Image.open(os.path.join(path.replace('images512x512', 'fgmasks512x512'), name)))
    assert np.array_equal(image['image'][3], np.where(mask > 127, 255, 127).astype(np.uint8))
    assert image['uv'].shape == (7, 8, 8) and image['uv'].dtype == np.float32
    stem = os.path.join(path.replace('images512x512', 'uvRender256x256'), name.split('.')[0])
    tex = np.asarray(PIL.Image.open(stem + '_uvgttex.png')).astype(np.float32) / 127.5 - 1
    pv = np.load(stem + '.npy').astype(np.float32)
    pv[..., -1] *= np.asarray(PIL.Image.open(tmp_path / dataset_new.UV_FACE_MASK)).astype(np.float32) / 255
    assert np.array_equal(image['uv'], np.concatenate([tex, pv], -1).transpose(2, 0, 1))
    assert np.array_equal(label_cam, np.concatenate([np.float32(labels[name]), np.float32(cams[name])]))
    orth = np.load(os.path.join(os.path.dirname(path), 'orthRender256x256_face_eye', name.split('.')[0] + '.npy'))
    assert vert['uvcoords_image'].shape == (8, 8, 3) and np.array_equal(vert['uvcoords_image'][..., :2], orth[..., :2])
    assert np.array_equal(vert['uvcoords_image'][..., 2], (orth[..., 2] >= 0.5).astype(np.float32))
    assert vert['mouths_mask'].tolist() == [0, 0, 1, 1] and vert['coeff'].dtype == np.float32 and vert['coeff'].shape == (20,)
    img2, lc2, v2 = ds.get_by_name(names[4])                                        # the drive loop's accessor (eval_seq.py:204)
    assert np.array_equal(img2['image'], image['image']) and np.array_equal(lc2, label_cam)
    assert np.array_equal(v2['uvcoords_image'], vert['uvcoords_image'])
    assert np.array_equal(ds.get_uvImg(4), image['uv']) and np.array_equal(ds.get_bgImg(4)[0], image['image'][3])
    flipped = dataset_new.ImageFolderDataset(**dict(_kwargs(path), return_name=False), xflip=True, max_size=4)
    assert len(flipped) == 8 and np.array_equal(flipped[5][0], flipped[1][0][:, :, ::-1])
    with pytest.raises(ValueError):
        ds.get_by_name('vidA/none.png')


READER_CONFIGS = (dict(load_uv=True), dict(load_bg=True), dict(load_uv=True, load_bg=True, resolution=8))


def _flatten(out, key, v):
    """One item of the reader as flat arrays: dicts and tuples by key / position under `key`, strings as 0-d str arrays."""
    if isinstance(v, dict):
        for k, x in v.items():
            _flatten(out, f'{key}/{k}', x)
    elif isinstance(v, (tuple, list)):
        for j, x in enumerate(v):
            _flatten(out, f'{key}/{j}', x)
    else:
        out[key] = np.array(v) if isinstance(v, str) else v


def test_equal_to_the_reference_reader(tmp_path, monkeypatch):
    """Item by item, dtype and shape included, equal to what the reference's class returns for the same directory in three reader
    configurations: tests/golden/dataset_reference.npz (tests/golden/make_golden.py:gen_dataset)."""
    path, names, _, _ = _write_dataset(tmp_path, rgba=True)
    monkeypatch.chdir(tmp_path)
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dataset_reference.npz'))
    for c, extra in enumerate(READER_CONFIGS):
        own = dataset_new.ImageFolderDataset(**_kwargs(path, **extra))
        assert len(own) == int(want[f'{c}/len'])
        assert str(list(own.label_shape)) == str(want[f'{c}/label_shape']) and str(list(own.image_shape)) == str(want[f'{c}/image_shape'])
        got = {}
        for i in range(len(own)):
            _flatten(got, f'{c}/item{i}', own[i])
            _flatten(got, f'{c}/by_name{i}', own.get_by_name(names[i]))
        keys = {k for k in want.files if k.startswith(f'{c}/') and k.split('/')[1] not in ('len', 'label_shape', 'image_shape')}
        assert set(got) == keys, (extra, sorted(set(got) ^ keys))
        for k in sorted(keys):
            a, b = want[k], np.asarray(got[k])
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (extra, k)
