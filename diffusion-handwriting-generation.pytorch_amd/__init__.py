"""MI355X-native reverse-diffusion handwriting sampler: a drop-in for the reference's
``DiffusionModel.forward`` and the ``infer`` sampling loop.  See DESIGN.md / INTEGRATION.md."""
from . import spec  # noqa: F401
from .checkpoint import find_checkpoint, load_model, read_config, read_state_dict  # noqa: F401
from .inference import Alignment, align, align_file, align_monotone, attention, ddim_levels, default_levels, get_alpha_set, get_beta_set, infer, infer_batch, infer_file, infer_file_batch, invert, load_style, null_condition, pad_strokes, read_img, remove_whitespace, restyle, restyle_file, rewrite_mask, sample, sample_ddim, score, score_file, slerp, token_spans, transfer, wrap_text, write_page, write_page_file  # noqa: F401
from .vector import StrokePaths, page_svg, save_page_svg, stroke_paths  # noqa: F401
from .truth import GroupBoxes, PageTruth, TruthItem, TruthLine, group_boxes, monotone_tokens, page_truth, save_page_truth, truth_json, word_map  # noqa: F401
from .vis import render_page, render_strokes, save_line_png, save_page_png, show_strokes, strokes_to_polylines  # noqa: F401
from .encode import encode_strokes, make_batches, padded_lengths, read_strokes_xml  # noqa: F401
from .imgprep import load_styles, prepare_images  # noqa: F401
from .quality import FeatureSet, FeatureStats, frechet_distance, kernel_distance, knn_radius, line_features, nearest, precision_recall, sample_metrics, sample_quality  # noqa: F401
from .dtw import dtw_distance, nearest_strokes, stroke_features  # noqa: F401
from .model import DiffusionModel, DiffusionWriter  # noqa: F401
from .style_extractor import StyleExtractor  # noqa: F401
from .tokenizer import Tokenizer, stroke_length  # noqa: F401
from . import train, train_model  # noqa: F401
