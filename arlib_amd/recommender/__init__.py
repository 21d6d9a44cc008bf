from .DirectAU import DirectAU  # noqa: F401  (the one model without a counterpart file in the reference's recommender/)

__all__ = ['DirectAU']
