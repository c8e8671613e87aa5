"""FREEDOM's public surface that needs no GPU: the registry entry and the model config."""


def test_freedom_registry_entry():
    from gmr.utils import _MODELS, get_trainer
    from gmr.trainer import Trainer
    assert _MODELS["FREEDOM"] == "freedom"
    assert get_trainer("FREEDOM") is Trainer


def test_freedom_yaml_loads():
    from gmr.configurator import Config
    cfg = Config("FREEDOM", "baby")
    assert cfg["embedding_size"] == 64 and cfg["feat_embed_dim"] == 64
    assert cfg["n_mm_layers"] == 1 and cfg["n_ui_layers"] == 2 and cfg["knn_k"] == 10
    assert cfg["mm_image_weight"] == 0.1 and cfg["dropout"] == 0.9 and cfg["reg_weight"] == 0.001
    for k in ("lambda_coeff", "cf_model", "degree_ratio", "weight_size"):  # read and ignored, as the reference
        assert cfg[k] is not None
