"""Drop-in surface of ``advchain.augmentor`` (reference: advchain/augmentor/__init__.py:1-7)."""
from .adv_transformation_base import AdvTransformBase  # noqa: F401
from .adv_noise import AdvNoise  # noqa: F401
from .adv_bias import AdvBias, bspline_kernel_2d, bspline_kernel_3d  # noqa: F401
from .adv_morph import (AdvMorph, get_base_grid, calculate_image_diff, calculate_jacobian_determinant,  # noqa: F401
                        integrate_by_add, vectorFieldExponentiation2D, vectorFieldExponentiation3D, applyComposition2D,
                        applyComposition3D, calculate_image_diff3D, calculate_jacobian_determinant3D,
                        jacobian_folding_stats)
from .adv_affine import AdvAffine  # noqa: F401
from .adv_compose_solver import ComposeAdversarialTransformSolver, calc_segmentation_consistency  # noqa: F401

__all__ = ["AdvTransformBase", "AdvNoise", "AdvBias", "AdvMorph", "AdvAffine",
           "ComposeAdversarialTransformSolver", "get_base_grid",
           "calculate_image_diff", "calculate_jacobian_determinant", "integrate_by_add",
           "vectorFieldExponentiation2D", "vectorFieldExponentiation3D", "applyComposition2D", "applyComposition3D",
           "bspline_kernel_2d", "bspline_kernel_3d", "calc_segmentation_consistency",
           "calculate_image_diff3D", "calculate_jacobian_determinant3D", "jacobian_folding_stats"]
