"""s4g_release_amd -- MI355X-native PointNet++ SA/FP hot path of S4G.

(The task names the package ``s4g-release_amd``; a hyphen cannot be imported,
so the importable spelling uses an underscore.)

Importing the package does not touch the GPU and does not load the HIP library;
the first operator call does, and fails loudly if ``libs4g_hip.so`` is absent.

The baselines' path ends in two consumers of `label_baseline_view`: `score_projections` (GPD on the projection maps)
and `score_close_regions` (PointNetGPD on the packed close-region point sets, each set whole and at its true size).
"""
__version__ = "0.1.0"


def accelerate(net, precision="f16x2"):
    """Run every SharedMLP and SA max-pool of `net` (any PointNet++ graph, the reference's own instances included) on
    the HIP contraction kernels; returns the qualified names of the converted modules.  See `accelerated.py`."""
    from .accelerated import accelerate as _accelerate
    return _accelerate(net, precision)


def grade_local_search(*args, **kwargs):
    """The data generator's per-frame local grasp search for every frame of every scene in one call: the S4G labels.
    See `postprocess.grade_local_search`."""
    from .postprocess import grade_local_search as _grade
    return _grade(*args, **kwargs)


def estimate_frames(*args, **kwargs):
    """The data generator's Darboux frames for every frame of every scene in one call.  See
    `postprocess.estimate_frames`."""
    from .postprocess import estimate_frames as _estimate
    return _estimate(*args, **kwargs)


def match_normals(*args, **kwargs):
    """The data generator's normal matching: every view point takes the mean normal of its nearest dense-scene points,
    for every scene in one call.  See `postprocess.match_normals`."""
    from .postprocess import match_normals as _match
    return _match(*args, **kwargs)


def estimate_normals(*args, **kwargs):
    """The reference's normal estimation (open3d's hybrid-search plane fit, turned towards the camera) for every point
    of every cloud in one call.  See `postprocess.estimate_normals`."""
    from .postprocess import estimate_normals as _estimate
    return _estimate(*args, **kwargs)


def label_view(*args, **kwargs):
    """View cloud in, S4G labels out: `match_normals` where asked for, the sampled indices, `estimate_frames` and
    `grade_local_search` in one call.  See `postprocess.label_view`."""
    from .postprocess import label_view as _label
    return _label(*args, **kwargs)


def grade_contact_frames(*args, **kwargs):
    """The contact model's grading of every scene frame of every scene in one call.  See
    `postprocess.grade_contact_frames`."""
    from .postprocess import grade_contact_frames as _grade
    return _grade(*args, **kwargs)


def label_contact_view(*args, **kwargs):
    """View cloud in, contact-model labels out: `match_nearest`, the frames of every scene point and the per-point
    fold over the graded scene frames in one call.  See `postprocess.label_contact_view`."""
    from .postprocess import label_contact_view as _label
    return _label(*args, **kwargs)


def contact_pairs(*args, **kwargs):
    """The antipodal point pairs of every object cloud of a batch in one call.  See `postprocess.contact_pairs`."""
    from .postprocess import contact_pairs as _pairs
    return _pairs(*args, **kwargs)


def grade_contact_pairs(*args, **kwargs):
    """The rolled frames of every pair graded over its object, the kept frames and the object point of each.  See
    `postprocess.grade_contact_pairs`."""
    from .postprocess import grade_contact_pairs as _grade
    return _grade(*args, **kwargs)


def label_contact_object(*args, **kwargs):
    """Object cloud in, the contact model's per-object frames out: `contact_pairs` and `grade_contact_pairs` in one
    call.  See `postprocess.label_contact_object`."""
    from .postprocess import label_contact_object as _label
    return _label(*args, **kwargs)


def compose_contact_scene(*args, **kwargs):
    """The per-object frames of posed objects as one scene for `grade_contact_frames` / `label_contact_view`.  See
    `postprocess.compose_contact_scene`."""
    from .postprocess import compose_contact_scene as _compose
    return _compose(*args, **kwargs)


def match_scene_frames(*args, **kwargs):
    """Every view point's frame, scores and recommended placements, looked up at its nearest point of a
    `DarbouxScene`.  See `postprocess.match_scene_frames`."""
    from .postprocess import match_scene_frames as _match
    return _match(*args, **kwargs)


def grade_precomputed_frames(*args, **kwargs):
    """The collision check of the recommended placements of candidate frames against the dense scene.  See
    `postprocess.grade_precomputed_frames`."""
    from .postprocess import grade_precomputed_frames as _grade
    return _grade(*args, **kwargs)


def label_precomputed_view(*args, **kwargs):
    """View cloud and `DarbouxScene` in, the curvature model's labels out: `match_scene_frames` and
    `grade_precomputed_frames` in one call, the view stage of the fast pipeline.  See
    `postprocess.label_precomputed_view`."""
    from .postprocess import label_precomputed_view as _label
    return _label(*args, **kwargs)


def best_placement(*args, **kwargs):
    """The baseline data generator's best placement per frame of a `LocalSearch`.  See `postprocess.best_placement`."""
    from .postprocess import best_placement as _best
    return _best(*args, **kwargs)


def close_regions(*args, **kwargs):
    """The packed close-region point sets and 12-channel projection maps of every frame of every scene in one call: the
    inputs of PointNetGPD and GPD.  See `postprocess.close_regions`."""
    from .postprocess import close_regions as _regions
    return _regions(*args, **kwargs)


def label_baseline_view(*args, **kwargs):
    """Frames in, baseline inputs out: `grade_local_search` without the label gate, `best_placement` and
    `close_regions` in one call.  See `postprocess.label_baseline_view`."""
    from .postprocess import label_baseline_view as _label
    return _label(*args, **kwargs)


def grade_precomputed_baseline_frames(*args, **kwargs):
    """The fast baseline labels' collision check and best-placement fold of candidate frames against the dense scene.
    See `postprocess.grade_precomputed_baseline_frames`."""
    from .postprocess import grade_precomputed_baseline_frames as _grade
    return _grade(*args, **kwargs)


def label_precomputed_baseline_view(*args, **kwargs):
    """View cloud and `DarbouxScene` in, the inputs of GPD and PointNetGPD out: `match_scene_frames` with the search
    threshold off, `grade_precomputed_baseline_frames` and `close_regions` of the view in one call.  See
    `postprocess.label_precomputed_baseline_view`."""
    from .postprocess import label_precomputed_baseline_view as _label
    return _label(*args, **kwargs)


def grade_eval_view_frames(*args, **kwargs):
    """The evaluation data's view search: per frame the first collision-free placement against the view cloud itself.
    See `postprocess.grade_eval_view_frames`."""
    from .postprocess import grade_eval_view_frames as _grade
    return _grade(*args, **kwargs)


def grade_eval_scene_frames(*args, **kwargs):
    """The evaluation data's ground truth: collision, single-label and antipodal score of poses against the dense
    labelled scene.  See `postprocess.grade_eval_scene_frames`."""
    from .postprocess import grade_eval_scene_frames as _grade
    return _grade(*args, **kwargs)


def label_eval_view(*args, **kwargs):
    """Rendered view and dense labelled scene in, the baselines' candidate grasps, classifier inputs and ground truth
    out: `estimate_frames`, `grade_eval_view_frames`, `close_regions` and `grade_eval_scene_frames` in one call.  See
    `postprocess.label_eval_view`."""
    from .postprocess import label_eval_view as _label
    return _label(*args, **kwargs)


def score_projections(*args, **kwargs):
    """GPD's grasp logits of the frames of `label_baseline_view`, read from its maps in place.  See
    `postprocess.score_projections`."""
    from .postprocess import score_projections as _score
    return _score(*args, **kwargs)


def build_gpd(*args, **kwargs):
    """The GPD baseline's classifier as a reference-shaped module.  See `baselines.build_gpd`."""
    from .baselines import build_gpd as _build
    return _build(*args, **kwargs)


def FusedGPD(*args, **kwargs):
    """`baselines.GPDClassifier` in eval mode on the HIP kernels.  See `baselines.FusedGPD`."""
    from .baselines import FusedGPD as _Fused
    return _Fused(*args, **kwargs)


def score_close_regions(*args, **kwargs):
    """PointNetGPD's grasp logits of the frames of `label_baseline_view`, read from its packed point sets in place.
    See `postprocess.score_close_regions`."""
    from .postprocess import score_close_regions as _score
    return _score(*args, **kwargs)


def build_pointnetgpd(*args, **kwargs):
    """The PointNetGPD baseline's classifier as a reference-shaped module.  See `baselines.build_pointnetgpd`."""
    from .baselines import build_pointnetgpd as _build
    return _build(*args, **kwargs)


def FusedPointNetGPD(*args, **kwargs):
    """`baselines.PointNetGPDClassifier` in eval mode on the HIP kernels.  See `baselines.FusedPointNetGPD`."""
    from .baselines import FusedPointNetGPD as _Fused
    return _Fused(*args, **kwargs)


def build_loss(*args, **kwargs):
    """(loss, metric) of a `MODEL.TYPE`: the networks' training objective and metric on one fused HIP call.  See
    `losses.build_loss`."""
    from .losses import build_loss as _build
    return _build(*args, **kwargs)


def PointNet2Loss(*args, **kwargs):
    """The curvature model's objective.  See `losses.PointNet2Loss`."""
    from .losses import PointNet2Loss as _Loss
    return _Loss(*args, **kwargs)


def PointNet2Metric(*args, **kwargs):
    """The curvature model's metric.  See `losses.PointNet2Metric`."""
    from .losses import PointNet2Metric as _Metric
    return _Metric(*args, **kwargs)


def ContactPointNet2Loss(*args, **kwargs):
    """The contact and edge models' objective.  See `losses.ContactPointNet2Loss`."""
    from .losses import ContactPointNet2Loss as _Loss
    return _Loss(*args, **kwargs)


def ContactPointNet2Metric(*args, **kwargs):
    """The contact and edge models' metric.  See `losses.ContactPointNet2Metric`."""
    from .losses import ContactPointNet2Metric as _Metric
    return _Metric(*args, **kwargs)
