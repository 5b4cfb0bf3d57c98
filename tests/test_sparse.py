"""Sparse slides on the GPU: cae_tile_byte_hist (csrc/cae_tiles.hip) against numpy.bincount, integer for integer, and
what zarrio builds on it -- compress_image with a mask, and decompress_image / segment_image on a store with skipped chunks.

Every expected number is restated here in numpy from the image, the mask and the labels; chunk bytes are the codec's own
(codec.encode of the padded chunk), as in tests/test_zarrio.py.
"""
import json
import os

import numpy as np
import pytest
import torch

from residue import poisoned_alloc  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (7, 9, 3), (16, 16, 3), (50, 100, 4), (264, 265, 3)]
CAPPED = (2000, 2000, 3)  # three such tiles: the launch is at its cap, and a block's span is twice the least and more
KINDS = ('random', 'equal', 'mostly', 'two')
I32 = 2 ** 31 - 1


def _tissue():
    from cnn_autoencoder_amd import tissue
    assert torch.cuda.is_available(), 'GPU tests need a HIP device'
    return tissue


# ----------------------------------------------------------------------------------------------------- histograms
def draw(kind, shape, rng):
    if kind == 'random':
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == 'equal':
        return np.full(shape, 240, dtype=np.uint8)
    if kind == 'mostly':  # 99 % at one value: a slide's background
        return np.where(rng.random(shape) < 0.99, 238, rng.integers(0, 256, shape)).astype(np.uint8)
    return rng.choice(np.array([0, 255], dtype=np.uint8), shape)


def extents_of(kind, n, h, w):
    if kind == 'full':
        return None
    if kind == 'ragged':
        return [(max(1, 2 * h // 3), max(1, 3 * w // 5))] * n
    if kind == 'empty':
        return [((0, w), (h, 0), (0, 0))[i % 3] for i in range(n)]
    if kind == 'per_tile':
        return [(max(h - i, 0), max(1, w // (i + 1))) for i in range(n)]
    return [((h + 5, w + 1000), (-3, w), (I32, I32))[i % 3] for i in range(n)]  # out of range: clamped to the tile


def bincounts(tiles, extents):
    n, h, w, c = tiles.shape
    out = np.zeros((n, 256), dtype=np.int64)
    sums = np.zeros(n, dtype=np.int64)
    for i in range(n):
        rows, cols = (h, w) if extents is None else (min(max(extents[i][0], 0), h), min(max(extents[i][1], 0), w))
        out[i] = np.bincount(tiles[i, :rows, :cols].ravel(), minlength=256)
        sums[i] = rows * cols * c
    return out, sums


def on_device(data, off):
    """the tiles `data` on the device, starting `off` bytes behind a 16-byte aligned address"""
    base = torch.empty(data.size + 64, dtype=torch.uint8, device='cuda')
    view = base[off:off + data.size].view(data.shape)
    view.copy_(torch.from_numpy(data))
    assert view.is_contiguous() and (view.data_ptr() - off) % 16 == 0
    return view


@pytest.mark.parametrize('shape', SHAPES)
def test_histograms_are_numpys_bincounts(shape, poisoned_alloc):  # noqa: F811
    """every shape with 1 and 3 tiles, at byte offsets 0, 1 and 3, for spread and concentrated bytes and every kind of
    extent; histogram and workspace come poisoned from the allocator, between guard bands"""
    T = _tissue()
    h, w, c = shape
    rng = np.random.default_rng(h * w + c)
    for n in (1, 3):
        for kind in KINDS:
            data = draw(kind, (n, h, w, c), rng)
            for off in (0, 1, 3):
                tiles = on_device(data, off)
                for ext in ('full', 'ragged', 'empty', 'per_tile', 'out_of_range'):
                    extents = extents_of(ext, n, h, w)
                    got = T.tile_histograms(tiles, extents).cpu().numpy()
                    want, sums = bincounts(data, extents)
                    assert got.dtype == np.int64 and got.shape == (n, 256)
                    assert np.array_equal(got, want), (n, kind, off, ext)
                    assert np.array_equal(got.sum(axis=1), sums), (n, kind, off, ext)
    assert poisoned_alloc.check() > 0


def test_histograms_where_the_launch_is_capped(poisoned_alloc):  # noqa: F811
    """three tiles of 12 MB: cae_tile_byte_hist_blocks gives each a third of the launch's cap, so a block walks a span of
    17 KiB and more, five turns of its 256 lanes, where an uncapped launch gives it 8 KiB; concentrated and spread bytes,
    aligned and not, whole and ragged"""
    from cnn_autoencoder_amd import _lib
    T = _tissue()
    h, w, c = CAPPED
    L = _lib.lib()
    bx = L.cae_tile_byte_hist_blocks(3, h, w, c)
    assert bx == 2048 // 3 and h * w * c / bx > 2 * 8192  # fewer blocks than spans of the least size: the cap holds
    assert L.cae_tile_byte_hist_blocks(1, h, w, c) > bx
    rng = np.random.default_rng(7)
    for kind, off, ext in (('random', 0, 'full'), ('mostly', 3, 'ragged'), ('two', 1, 'per_tile'), ('equal', 0, 'full')):
        data = draw(kind, (3, h, w, c), rng)
        extents = extents_of(ext, 3, h, w)
        got = T.tile_histograms(on_device(data, off), extents).cpu().numpy()
        want, sums = bincounts(data, extents)
        assert np.array_equal(got, want), (kind, off, ext)
        assert np.array_equal(got.sum(axis=1), sums)
    assert poisoned_alloc.check() > 0


def test_a_small_call_after_a_large_one_on_the_same_buffers():
    """nothing of the large call's partials or counts is in the small call's result, and the small call writes its own
    rows only"""
    from cnn_autoencoder_amd import _lib
    _tissue()
    L = _lib.lib()
    rng = np.random.default_rng(3)
    large, small = draw('random', (3, 264, 265, 3), rng), draw('mostly', (1, 7, 9, 3), rng)
    ws_bytes = L.cae_tile_byte_hist_workspace(3, 264, 265, 3)
    assert L.cae_tile_byte_hist_workspace(1, 7, 9, 3) < ws_bytes
    ws = torch.full((ws_bytes // 8,), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device='cuda')
    hist = torch.full((3, 256), 0x7F7F7F7F7F7F7F7F, dtype=torch.int64, device='cuda')

    def run(data):
        t = on_device(data, 0)
        n, h, w, c = data.shape
        _lib.check(L.cae_tile_byte_hist(t.data_ptr(), None, n, h, w, c, hist.data_ptr(), ws.data_ptr(),
                                        L.cae_tile_byte_hist_workspace(n, h, w, c), _lib.stream_ptr()))
        return hist.cpu().numpy()

    after_large = run(large)
    assert np.array_equal(after_large, bincounts(large, None)[0])
    after_small = run(small)
    assert np.array_equal(after_small[:1], bincounts(small, None)[0])
    assert np.array_equal(after_small[1:], after_large[1:])
    with pytest.raises(ValueError, match='workspace'):
        _lib.check(L.cae_tile_byte_hist(hist.data_ptr(), None, 3, 264, 265, 3, hist.data_ptr(), ws.data_ptr(), ws_bytes - 1,
                                        _lib.stream_ptr()))


def test_the_wrapper_refuses_what_the_kernel_does_not_read():
    T = _tissue()
    tiles = torch.zeros((2, 8, 9, 3), dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='contiguous'):
        T.tile_histograms(tiles.permute(0, 2, 1, 3))
    with pytest.raises(ValueError, match='extent'):
        T.tile_histograms(tiles, [(1, 2)])
    with pytest.raises(ValueError, match='extent'):
        T.tile_histograms(tiles, np.ones((2, 2)))
    none = T.tile_histograms(tiles[:0])
    assert none.shape == (0, 256) and none.dtype == torch.int64 and none.is_cuda
    got = T.tile_histograms(tiles, torch.tensor([[8, 9], [2, 2]]))
    assert got[:, 0].tolist() == [216, 12] and int(got[:, 1:].sum()) == 0


# ---------------------------------------------------------------------------------------------------- the stores
P = 64


def colour_state(cfg, seed):
    """a synthetic checkpoint with seeded colour layers, so that the store reads at reduced scales too"""
    from cnn_autoencoder_amd import synth
    cfg = dict(cfg, multiscale_analysis=True)
    state = synth.synthetic_state(cfg, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    k, c_net, c_org = cfg.get('kernel_size', 3), cfg['channels_net'], cfg['channels_org']
    b = synth._xavier_bound(c_net, c_org, k)
    for i in range(cfg['compression_level'] - 1):
        state['decoder'][f'color_layers.{i}.0.weight'] = torch.from_numpy(
            rng.uniform(-b, b, (c_org, c_net, k, k)).astype(np.float32))
    return state


@pytest.fixture
def checkpoint(tmp_path):
    from cnn_autoencoder_amd import synth
    path = str(tmp_path / 'ckpt.pth')
    torch.save(colour_state(dict(synth.CANONICAL, channels_net=32, channels_bn=48, compression_level=3), 4), path)
    return path


def slide_image():
    """170 x 230 x 3 (3 x 4 chunks of 64, ragged): flat 240, tissue in chunks (0, 1) and (1, 2), a black 10 x 10 mark in
    the background chunk (2, 0); the mask at 1 / 32 covers exactly the two tissue chunks"""
    from cnn_autoencoder_amd import synth
    img = np.full((170, 230, 3), 240, dtype=np.uint8)
    img[0:64, 64:128] = synth.histo_tile(P, 2)
    img[64:128, 128:192] = synth.histo_tile(P, 5)
    img[140:150, 10:20] = 0
    mask = np.zeros((6, 8), dtype=bool)
    mask[0:2, 2:4] = True
    mask[2:4, 4:6] = True
    return img, mask


def chunk_files(store, group='0/0'):
    root = os.path.join(store, *group.split('/'))
    return sorted(f for f in os.listdir(root) if not f.startswith('.'))


def tree(store):
    out = {}
    for root, _, files in os.walk(store):
        for f in files:
            out[os.path.relpath(os.path.join(root, f), store)] = open(os.path.join(root, f), 'rb').read()
    return out


def best_fill(samples):
    """the fill value of the contract from the samples themselves: every f tried in int64"""
    v = samples.astype(np.int64)
    sse = [int(((v - f) ** 2).sum()) for f in range(256)]
    return sse.index(min(sse)), min(sse)


def test_a_sparse_store(tmp_path, checkpoint):
    import cnn_autoencoder_amd as cae
    from cnn_autoencoder_amd import tissue, zarrio
    _tissue()
    img, mask = slide_image()
    keep = tissue.mask_tiles(mask, 1 / 32, img.shape, (P, P))
    kept = [(0, 1), (1, 2)]
    assert sorted(zip(*np.nonzero(keep))) == kept
    store = str(tmp_path / 'sparse.zarr')
    z = zarrio.compress_image('CAE', checkpoint, img, store, patch_size=P, batch_tiles=4, mask=mask, mask_scale=1 / 32)
    tiles = z.chunk_indices()
    assert len(tiles) == 12
    cand = [i for i in tiles if (i[0], i[1]) not in kept]
    samples = np.concatenate([img[z.chunk_slices(i)].ravel() for i in cand])
    fill, sse = best_fill(samples)
    # 300 samples of the mark at 0 among 92 724 at 240: the mean is 239.2, so the best fill value is 239 and every other
    # sample is one level off
    n_marked = 42 * 64 * 3
    marked_sse = 300 * 239 ** 2 + (n_marked - 300)
    assert fill == 239 and sse == marked_sse + (samples.size - n_marked)
    # metadata
    meta = json.load(open(os.path.join(store, '0', '0', '.zarray')))
    assert meta['fill_value'] == fill and z.fill_value == fill
    attrs = json.load(open(os.path.join(store, '0', '0', '.zattrs')))
    assert attrs == dict(sparse=dict(fill_value=fill, tiles=12, kept=2, rescued=0, skipped=10, skipped_samples=int(samples.size),
                                     skipped_sse=sse))
    assert samples.size == 170 * 230 * 3 - 2 * P * P * 3
    # chunk files: exactly the kept chunks, each the codec's bytes of the padded chunk
    assert chunk_files(store) == ['0.1.0', '1.2.0']
    codec = cae.ConvolutionalAutoencoder(checkpoint=checkpoint)
    for i, j in kept:
        assert z.read_chunk_bytes((i, j, 0)) == codec.encode(z.pad_chunk(img[z.chunk_slices((i, j, 0))]))
    # readers: the pipelined read is the chunk-by-chunk read, and the fill value wherever a chunk was skipped
    zo = zarrio.ZarrArray.open(store, '0/0')
    assert zo.is_sparse
    rec = zarrio.decompress_image(store, batch_tiles=4)
    assert rec.shape == img.shape and rec.dtype == np.uint8 and np.array_equal(rec, zo[:])
    for idx in cand:
        assert (rec[zo.chunk_slices(idx)] == fill).all(), idx
    for i, j in kept:
        assert np.array_equal(rec[zo.chunk_slices((i, j, 0))], codec.decode(z.read_chunk_bytes((i, j, 0))))
    assert np.array_equal(zarrio.decompress_image(store, roi=(100, 170, 0, 100)), rec[100:170, 0:100])
    assert np.array_equal(zarrio.decompress_image(store, roi=(10, 100, 60, 200)), rec[10:100, 60:200])
    # at half the resolution: fill-value tiles of half the size, the kept chunks as the codec decodes them at that scale
    half = zarrio.decompress_image(store, scale=1, batch_tiles=4)
    assert half.shape == (85, 115, 3)
    want = np.full((96, 128, 3), fill, dtype=np.uint8)
    for i, j in kept:
        want[i * 32:(i + 1) * 32, j * 32:(j + 1) * 32] = codec.decode_batch([z.read_chunk_bytes((i, j, 0))], scale=1)[0]
    assert np.array_equal(half, want[:85, :115])

    # the guard: below the marked chunk's RMSE that chunk is coded after all, into the store that has no file for it yet
    rmse = (marked_sse / n_marked) ** 0.5
    z2 = zarrio.compress_image('CAE', checkpoint, img, store, patch_size=P, batch_tiles=4, mask=mask, mask_scale=1 / 32,
                               max_fill_rmse=rmse * 0.999)
    assert chunk_files(store) == ['0.1.0', '1.2.0', '2.0.0']
    assert z2.attrs['sparse'] == dict(fill_value=fill, tiles=12, kept=2, rescued=1, skipped=9,
                                      skipped_samples=int(samples.size) - n_marked, skipped_sse=sse - marked_sse)
    assert z2.fill_value == fill
    padded = z2.pad_chunk(img[z2.chunk_slices((2, 0, 0))])
    assert (padded[42:] == fill).all()  # an edge chunk is padded with the fill value, as zarr pads
    assert z2.read_chunk_bytes((2, 0, 0)) == codec.encode(padded)
    rec2 = zarrio.decompress_image(store, batch_tiles=4)
    assert np.array_equal(rec2, zarrio.ZarrArray.open(store, '0/0')[:])
    assert np.array_equal(rec2[128:170, 0:64], codec.decode(z2.read_chunk_bytes((2, 0, 0)))[:42])
    # at (just above) that RMSE it is skipped again, and its stale file goes
    z3 = zarrio.compress_image('CAE', checkpoint, img, store, patch_size=P, batch_tiles=4, mask=mask, mask_scale=1 / 32,
                               max_fill_rmse=rmse * 1.001)
    assert chunk_files(store) == ['0.1.0', '1.2.0'] and z3.attrs['sparse'] == attrs['sparse']

    # a given fill value without a guard: no candidate is looked at, so nothing is known about the loss
    z4 = zarrio.compress_image('CAE', checkpoint, img, store, patch_size=P, batch_tiles=4, mask=mask, mask_scale=1 / 32,
                               fill_value=200)
    assert z4.attrs['sparse'] == dict(fill_value=200, tiles=12, kept=2, rescued=0, skipped=10, skipped_samples=None,
                                      skipped_sse=None)
    assert json.load(open(os.path.join(store, '0', '0', '.zarray')))['fill_value'] == 200
    rec4 = zarrio.decompress_image(store, batch_tiles=4)
    assert (rec4[128:, :64] == 200).all() and np.array_equal(rec4[0:64, 64:128], rec[0:64, 64:128])
    # a given fill value with a guard: the loss against that value, exactly
    z5 = zarrio.compress_image('CAE', checkpoint, img, store, patch_size=P, batch_tiles=4, mask=mask, mask_scale=1 / 32,
                               fill_value=239, max_fill_rmse=1.5)
    s5 = z5.attrs['sparse']
    assert (s5['rescued'], s5['skipped'], s5['skipped_samples']) == (1, 9, int(samples.size) - n_marked)
    assert s5['skipped_sse'] == s5['skipped_samples']  # every skipped sample is 240: one level from 239


def test_without_the_new_arguments_nothing_changes(tmp_path, checkpoint):
    from cnn_autoencoder_amd import zarrio
    _tissue()
    img, _ = slide_image()
    a, b = str(tmp_path / 'a.zarr'), str(tmp_path / 'b.zarr')
    zarrio.compress_image('CAE', checkpoint, img, a, patch_size=P, batch_tiles=4)
    zarrio.compress_image('CAE', checkpoint, img, b, patch_size=P, batch_tiles=4, mask=None, mask_scale=None,
                          fill_value=None, max_fill_rmse=None)
    ta, tb = tree(a), tree(b)
    assert sorted(ta) == sorted(tb) and len(chunk_files(a)) == 12 and ta == tb
    assert not any(k.endswith('.zattrs') for k in ta)
    assert json.loads(ta[os.path.join('0', '0', '.zarray')])['fill_value'] == 0
    assert not zarrio.ZarrArray.open(a, '0/0').is_sparse
    # a store that is not sparse and misses a chunk file is damaged, as ever
    os.remove(os.path.join(a, '0', '0', '1.1.0'))
    with pytest.raises(ValueError, match='missing chunk file'):
        zarrio.decompress_image(a, batch_tiles=4)


# ------------------------------------------------------------------------------------------------- segmentation
SEG_CODEC = dict(channels_net=24, channels_bn=16, compression_level=3)


def seg_head(classes, seed=0):
    from cnn_autoencoder_amd import segmenters
    torch.manual_seed(seed)
    m = segmenters.JNet(**dict(SEG_CODEC, seg_channels_net=6, seg_channels_bn=20, num_classes=classes, concat_bridges=True,
                               batch_norm=True))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.GroupNorm):
                mod.weight.copy_(1.0 + 0.5 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.3 * torch.randn(mod.bias.shape, generator=g))
    return m.cuda().eval()


@pytest.mark.parametrize('classes', [1, 5])
def test_segment_image_on_a_sparse_store(tmp_path, classes):
    """128 x 192, 2 x 3 whole chunks, two of them kept: their records are those of the dense run of the same image, the
    skipped chunks' are made from the labels with the prediction 'background everywhere'"""
    from cnn_autoencoder_amd import segmenters, synth, zarrio
    _tissue()
    ckpt = str(tmp_path / 'ckpt.pth')
    torch.save(synth.synthetic_state(dict(synth.CANONICAL, **SEG_CODEC), seed=3), ckpt)
    seg = seg_head(classes)
    H, W = 128, 192
    img = np.full((H, W, 3), 240, dtype=np.uint8)
    img[0:64, 0:64] = synth.histo_tile(P, 1)
    img[64:128, 128:192] = synth.histo_tile(P, 3)
    mask = np.zeros((4, 6), dtype=bool)
    mask[0:2, 0:2] = True
    mask[2:4, 4:6] = True
    kept = [(0, 0), (1, 2)]
    labels = np.random.default_rng(5).integers(0, max(classes, 2) + 1, (H, W)).astype(np.uint8)
    dense, sparse = str(tmp_path / 'dense.zarr'), str(tmp_path / 'sparse.zarr')
    zarrio.compress_image('CAE', ckpt, img, dense, patch_size=P, batch_tiles=4)
    z = zarrio.compress_image('CAE', ckpt, img, sparse, patch_size=P, batch_tiles=4, mask=mask, mask_scale=1 / 32)
    assert chunk_files(sparse) == ['0.0.0', '1.2.0'] and z.attrs['sparse']['skipped'] == 4
    for store in (dense, sparse):
        zarrio.ZarrArray.create(store, 'labels/0', (H, W), (P, P), np.uint8, codec=zarrio.Zlib(1))[:] = labels
    out_d, out_s = str(tmp_path / 'pred_dense.zarr'), str(tmp_path / 'pred_sparse.zarr')
    want = zarrio.segment_image(dense, seg, out_d, target_group='labels/0', batch_tiles=4, scores=True)
    got = zarrio.segment_image(sparse, seg, out_s, target_group='labels/0', batch_tiles=4, scores=True)
    assert 'skipped_tiles' not in want and got['skipped_tiles'] == 4 and got['tiles'] == 6
    assert got['records'].shape == (6, 6) and got['records'].dtype == np.int64
    tiles = z.chunk_indices()
    for t, (i, j, _) in enumerate(tiles):
        if (i, j) in kept:
            assert np.array_equal(got['records'][t], want['records'][t]), (i, j)
        else:
            part = labels[i * P:(i + 1) * P, j * P:(j + 1) * P]
            zero, px = int((part == 0).sum()), P * P
            rule = (0, zero, 0, px - zero, px - zero, 0) if classes == 1 else (zero, 0, px - zero, px - zero, px, zero)
            assert got['records'][t].tolist() == list(rule), (i, j)
    for k, v in segmenters.class_metrics(got['records'].sum(axis=0), multiclass=classes > 1).items():
        assert got[k] == v, k
    # class maps and scores: chunks for the kept tiles only, and background wherever a chunk was skipped
    assert chunk_files(out_s, 'class/0/0') == ['0.0', '1.2'] and len(chunk_files(out_d, 'class/0/0')) == 6
    assert chunk_files(out_s, 'scores/0/0') == ['0.0.0', '0.1.2']
    cls_s, cls_d = zarrio.ZarrArray.open(out_s, 'class/0/0')[:], zarrio.ZarrArray.open(out_d, 'class/0/0')[:]
    for i, j, _ in tiles:
        sl = (slice(i * P, (i + 1) * P), slice(j * P, (j + 1) * P))
        assert np.array_equal(cls_s[sl], cls_d[sl]) if (i, j) in kept else not cls_s[sl].any(), (i, j)
    # without a target: no records, the same class map
    plain = zarrio.segment_image(sparse, seg, str(tmp_path / 'pred_plain.zarr'), batch_tiles=4)
    assert plain['skipped_tiles'] == 4 and 'records' not in plain
    assert np.array_equal(zarrio.ZarrArray.open(str(tmp_path / 'pred_plain.zarr'), 'class/0/0')[:], cls_s)
    # a skipped chunk has no logit: no curve and no object-level counts from a sparse store
    with pytest.raises(ValueError, match='sparse'):
        zarrio.segment_image(sparse, seg, str(tmp_path / 'x.zarr'), target_group='labels/0', object_level=True)
    if classes == 1:
        with pytest.raises(ValueError, match='sparse'):
            zarrio.segment_image(sparse, seg, str(tmp_path / 'x.zarr'), target_group='labels/0', roc_bits=14)
    # the dense store with one chunk file deleted is damaged, for both readers
    os.remove(os.path.join(dense, '0', '0', '0.1.0'))
    with pytest.raises(ValueError, match='missing chunk file'):
        zarrio.decompress_image(dense, batch_tiles=4)
    with pytest.raises(ValueError, match='missing chunk file'):
        zarrio.segment_image(dense, seg, str(tmp_path / 'y.zarr'), batch_tiles=4)
