"""predict_regions behind the drop-in classes (f32 tiny-8 tower, synthetic weights, the scenes and class file of
tests/test_gpu_sieve_route.py: 40 x 150 and 47 x 61, crop 32, stride 16, Q = 8 -> K = 5).

Its label maps must equal those of ``predict_many`` byte for byte, and its table tests/regions_reference.py applied to those labels,
exactly: plain, with ``min_region`` set (the regions of the sieved labels), with ``with_score`` (SCORE_Q against q of the gathered
probabilities) and with an ``ori_shape`` of another size."""
import numpy as np
import pytest
import torch

import regions_reference as G
import sieve_reference as S
from test_gpu_sieve_route import BG, DEV, SHAPES, choose_min_region, images, seg_of

pytestmark = pytest.mark.gpu


class Sample:
    """What predict fills: set_data stores the fields as attributes too, as mmengine's data elements do."""

    def __init__(self, meta):
        self.metainfo, self.data = meta, {}

    def set_data(self, d):
        self.data.update(d)
        self.__dict__.update(d)


def check(labels, regions, connectivity, min_area=1, skip=BG, confs=None, want_map=False):
    """One dict per image against the reference on that image's labels; the rows of an image count from 0."""
    assert len(labels) == len(regions)
    listed = 0
    for n, (lab, d) in enumerate(zip(labels, regions)):
        m = lab[0].cpu().numpy()
        rows, root = G.all_rows(m, connectivity, None if confs is None else confs[n])
        want, counts, region_of = G.assemble([(G.listed(rows, min_area, skip), root)])
        got = torch.stack([d[k] for k in ("root", "label", "area")], 1).cpu().numpy()
        assert np.array_equal(got, want[:, G.ROOT:G.AREA + 1]) and np.array_equal(d["bbox"].cpu().numpy(), want[:, G.Y0:G.X1 + 1]), n
        area = want[:, G.AREA].astype(np.float64)
        assert np.array_equal(d["centroid"].cpu().numpy(), want[:, G.SUM_Y:G.SUM_X + 1] / area[:, None]), n
        if confs is None:
            assert d["score"] is None
        else:
            assert np.array_equal(d["score_q"].cpu().numpy(), want[:, G.SCORE_Q]), n
            assert np.array_equal(d["score"].cpu().numpy(), want[:, G.SCORE_Q] / float(1 << 24) / area), n
        if want_map:
            assert d["region_of"].dtype == torch.int32 and np.array_equal(d["region_of"].cpu().numpy(), region_of[0]), n
        listed += len(want)
    assert listed > 0, "no region is listed: the case would show nothing"


@pytest.mark.parametrize("cls_name", ["SegmentorEx", "Segmentor"])
def test_labels_are_predict_many_and_the_table_is_the_reference(tmp_path_factory, cls_name):
    seg = seg_of(tmp_path_factory, cls_name)
    imgs = images()
    plain = seg.predict_many(imgs)
    labels, regions = seg.predict_regions(imgs)
    assert all(a.dtype == torch.int64 and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(labels, plain))
    check(labels, regions, 4)
    labels, regions = seg.predict_regions(imgs, min_area=5, include_bg=True, want_map=True)
    assert all(torch.equal(a, b) for a, b in zip(labels, plain))
    check(labels, regions, 4, min_area=5, skip=None, want_map=True)


def test_with_min_region_the_regions_of_the_sieved_labels(tmp_path_factory):
    imgs = images()
    m = choose_min_region(seg_of(tmp_path_factory).predict_many(imgs), 8)
    seg = seg_of(tmp_path_factory, min_region=m, region_connectivity=8)
    sieved = seg.predict_many(imgs)
    labels, regions = seg.predict_regions(imgs, include_bg=True)
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(labels, sieved))
    check(labels, regions, 8, skip=None)
    labels, regions = seg.predict_regions(imgs)
    check(labels, regions, 8)


@pytest.mark.parametrize("oris", [None, [(33, 170), SHAPES[1]]], ids=["own_size", "another_ori_shape"])
def test_data_samples_with_score(tmp_path_factory, oris):
    seg = seg_of(tmp_path_factory)
    imgs = images()
    oris = [tuple(x.shape[-2:]) for x in imgs] if oris is None else oris
    base = seg.predict_many(imgs, [Sample(dict(ori_shape=o)) for o in oris])
    samples = [Sample(dict(ori_shape=o)) for o in oris]
    labels, regions = seg.predict_regions(imgs, samples, with_score=True, want_map=True)
    assert [tuple(a.shape[-2:]) for a in labels] == oris
    confs = []
    for a, b, s, d in zip(labels, base, samples, regions):
        assert a.cpu().numpy().tobytes() == b.data["pred_sem_seg"].data.cpu().numpy().tobytes()
        assert torch.equal(s.data["pred_sem_seg"].data, b.data["pred_sem_seg"].data)
        assert torch.equal(s.data["seg_logits"].data, b.data["seg_logits"].data)
        assert s.data["pred_regions"] is d
        confs.append(b.data["seg_logits"].data.gather(0, a)[0].cpu().numpy())  # the probability of the pixel's final label
    check(labels, regions, 4, confs=confs, want_map=True)
    # without the score the labels-only call's dicts carry none
    labels, regions = seg.predict_regions(imgs, [Sample(dict(ori_shape=o)) for o in oris])
    check(labels, regions, 4)


def test_with_score_without_data_samples(tmp_path_factory):
    """The probability tail at the images' own sizes: the labels and scores of the call with data samples of those sizes."""
    seg = seg_of(tmp_path_factory)
    imgs = images()
    base = seg.predict_many(imgs, [Sample(dict(ori_shape=tuple(x.shape[-2:]))) for x in imgs])
    labels, regions = seg.predict_regions(imgs, with_score=True)
    confs = []
    for a, b in zip(labels, base):
        assert a.cpu().numpy().tobytes() == b.data["pred_sem_seg"].data.cpu().numpy().tobytes()
        confs.append(b.data["seg_logits"].data.gather(0, a)[0].cpu().numpy())
    check(labels, regions, 4, confs=confs)


def test_whole_image_inference(tmp_path_factory):
    """slide_crop <= 0 has no flush groups: one call per image, labels those of predict_many, with and without the score."""
    seg = seg_of(tmp_path_factory, "Segmentor", slide_crop=0)
    xs = [images()[1][:, :40, :48].contiguous(), images()[0][:, :32, :64].contiguous()]
    plain = seg.predict_many(xs)
    labels, regions = seg.predict_regions(xs, want_map=True)
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(labels, plain))
    check(labels, regions, 4, want_map=True)
    metas = [dict(ori_shape=tuple(x.shape[-2:])) for x in xs]
    base = [seg.predict(x[None], [Sample(mt)])[0] for x, mt in zip(xs, metas)]
    for samples in (None, [Sample(mt) for mt in metas]):
        labels, regions = seg.predict_regions(xs, samples, with_score=True)
        assert all(torch.equal(a, b.data["pred_sem_seg"].data) for a, b in zip(labels, base))
        check(labels, regions, 4, confs=[b.data["seg_logits"].data.gather(0, a)[0].cpu().numpy() for a, b in zip(labels, base)])


def test_a_final_label_outside_the_class_planes_scores_zero(tmp_path_factory):
    """The gather behind with_score (ops.label_confidence): a pixel whose label is no class plane contributes 0."""
    from clip_decontamination_amd import ops
    lab = torch.tensor([[0, 0, 7], [1, 1, -3]], dtype=torch.int64, device=DEV)[None]
    probs = torch.stack([torch.full((2, 3), 0.25, device=DEV), torch.full((2, 3), 0.5, device=DEV)])
    conf = ops.label_confidence(probs, lab)
    assert conf.shape == lab.shape and conf[0].tolist() == [[0.25, 0.25, 0.0], [0.5, 0.5, 0.0]]
    out = ops.regions(lab, conf, 4)
    assert out["label"].tolist() == [0, 7, 1, -3] and out["score"].tolist() == [0.25, 0.0, 0.5, 0.0]


def test_refusals(tmp_path_factory):
    from clip_decontamination_amd import pipeline as P
    seg = seg_of(tmp_path_factory)
    imgs = images()
    with pytest.raises(ValueError, match="min_area"):
        seg.predict_regions(imgs, min_area=0)
    seg.tile_group = "world"
    try:
        with pytest.raises(ValueError) as e:
            seg.predict_regions(imgs)
        assert str(e.value) == P.REGIONS_TILE_GROUP
    finally:
        seg.tile_group = None
