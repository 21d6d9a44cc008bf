from .DirectAU import DirectAU  # noqa: F401  (a model without a counterpart file in the reference's recommender/)
from .APR import APR  # noqa: F401  (likewise: the defended victim)
from .MultVAE import MultVAE  # noqa: F401  (likewise: the inductive victim)
from .iALS import iALS  # noqa: F401  (likewise: the ALS-trained WRMF victim)
from .ItemKNN import ItemKNN  # noqa: F401  (likewise: the neighbourhood victim of the shilling attacks)
from .UserKNN import UserKNN  # noqa: F401  (likewise: the user-based neighbourhood victim)

__all__ = ['DirectAU', 'APR', 'MultVAE', 'iALS', 'ItemKNN', 'UserKNN']
