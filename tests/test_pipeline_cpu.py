"""pipeline.py without a device: the names evaluate.py hands on, and the one function that routes a pair through a1-a5."""
import inspect
import itertools
from types import SimpleNamespace

MOVED = ("_PinnedRing", "_ring", "_index_tensor", "_to_host", "_phase_a", "PairBatch", "PairResult", "_phase_b",
         "_draw_keypoints_host", "_draw_keypoints", "register_pair", "RegistrationPipeline")


def test_evaluate_hands_on_the_same_objects():
    from umeregrobust_amd import evaluate, pipeline
    for name in MOVED:
        assert getattr(evaluate, name) is getattr(pipeline, name), name
    # what stays is defined in evaluate.py and resolves its helpers through evaluate's own globals (tests replace them there)
    for name in ("evaluate_pairs", "select_hypothesis", "pc_fcht", "prepare_selection", "refine_registration", "main"):
        assert getattr(evaluate, name).__module__ == evaluate.__name__ and not hasattr(pipeline, name), name
    assert evaluate.pc_fcht.__globals__["FeatureCorrelator"] is evaluate.FeatureCorrelator
    assert isinstance(evaluate._OVERLAP_STREAMS, dict) and not hasattr(pipeline, "_OVERLAP_STREAMS")


def test_phase_a_route_truth_table(monkeypatch):
    """phase_a_route against the three conditions it replaces, written out as they stood in register_pair, _phase_a and
    RegistrationPipeline._submit_slot: (timing given, materialize_D, f16r or not, Hungarian flag, pair present) in all 32 combinations,
    a present pair in both its forms, the Hungarian flag absent as well as False."""
    from umeregrobust_amd import ops, pipeline
    from umeregrobust_amd.pipeline import NATIVE, PER_CLOUD, STACKED, phase_a_route
    stacked, ragged = SimpleNamespace(pts=object()), SimpleNamespace(pts=None)
    n = 0
    for timing_given, materialize_D, f16r, hungarian, pair_present in itertools.product((False, True), repeat=5):
        timing = {} if timing_given else None
        monkeypatch.setattr(ops, "DEFAULT_MATCH_PRECISION", "f16r" if f16r else "f32")     # (read through the module at call time)
        for args in ([SimpleNamespace(hungarian_matching_flag=True)] if hungarian else
                     [SimpleNamespace(hungarian_matching_flag=False), SimpleNamespace()]):
            for pair in ((stacked, ragged) if pair_present else (None,)):
                # register_pair: builds a PairBatch (on the device: PairBatch.from_clouds itself returns None for a host tensor)
                src_pts = SimpleNamespace(is_cuda=True)
                builds = timing is None and not materialize_D and src_pts.is_cuda and ops.DEFAULT_MATCH_PRECISION == "f16r" \
                    and not getattr(args, "hungarian_matching_flag", False)
                assert (phase_a_route(args, timing, materialize_D, True) == NATIVE) == builds
                # _phase_a: the one native call, else the stacked launches for a stacked pair, else the per-cloud ones
                one_call = pair is not None and timing is None and not materialize_D and ops.DEFAULT_MATCH_PRECISION == "f16r" \
                    and not getattr(args, "hungarian_matching_flag", False)
                layered = STACKED if pair is not None and pair.pts is not None else PER_CLOUD
                assert phase_a_route(args, timing, materialize_D, pair) == (NATIVE if one_call else layered)
                # _submit_slot: the slot's graph (with the pipeline's own extras given: graphs on, no draw worker, the current device);
                # it calls _phase_a with materialize_D=False
                self = SimpleNamespace(use_graphs="slot", args=args, pool=None, dev=SimpleNamespace(index=0))
                current_device = 0
                graph = bool(self.use_graphs and pair is not None and timing is None and ops.DEFAULT_MATCH_PRECISION == "f16r"
                             and not getattr(self.args, "hungarian_matching_flag", False) and self.pool is None
                             and current_device == self.dev.index)
                assert (phase_a_route(self.args, timing, False, pair) == NATIVE) == graph
                n += 1
    assert n == 8 * (2 + 1) + 8 * 2 * (2 + 1)
    # _submit_slot builds the PairBatch of a pair that came without one on `timing is None` alone, as it did
    src = inspect.getsource(pipeline.RegistrationPipeline._submit_slot)
    assert "if timing is None:\n" in src and src.count("phase_a_route(") == 1
    # the condition itself stands once in the module
    assert inspect.getsource(pipeline).count('ops.DEFAULT_MATCH_PRECISION == "f16r"') == 1
