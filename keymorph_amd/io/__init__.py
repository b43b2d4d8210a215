"""On-disk formats and loader shims either side of the registration path: host-side
only -- no GPU code and no third-party readers (torchio / nibabel are not needed).  brain.py and centering.py are the
exceptions: the notebooks' brain-extraction and centering cells as calls, which run the package's GPU operators."""
from .checkpoint import load_checkpoint, save_checkpoint          # noqa: F401
from .nifti import read_nifti, write_nifti                        # noqa: F401
from .pairs import DATA, AFFINE, PairLoader, make_subject         # noqa: F401
from .groupwise import evaluate_group, save_dict_as_json         # noqa: F401
from .brain import extract_brain, load_brain_extractor         # noqa: F401
from .centering import center_to, estimate_translation, translate         # noqa: F401
from .intensity import (apply_mat, estimate_affine, estimate_rigid, mat_to_voxel, register_intensity,         # noqa: F401
                        rigid_params_to_voxel, rotation_matrix, voxel_to_mat)
from .bspline import apply_bspline, register_bspline         # noqa: F401
from .svf import apply_svf, register_svf, svf_grid         # noqa: F401
from .greedy import apply_greedy, register_greedy         # noqa: F401
