"""BandwagonAttack (reference attack/Black/BandwagonAttack.py:57-80): each fake user rates maliciousFeedbackNum // 2 random fillers, every
target and the maliciousFeedbackNum most popular items.  A target that is also popular is listed twice and sums to 2.0, as in the reference."""
import scipy.sparse as sp

from ._shilling import ShillingAttackModel, remaining_ids, filler_draw, fake_block


class BandwagonAttack(ShillingAttackModel):
    def posionDataAttack(self):
        selectItem = self.getPopularItemId(self.maliciousFeedbackNum)
        pool = remaining_ids(self.itemNum, self.targetItem, selectItem)
        rows = [filler_draw(pool, self.maliciousFeedbackNum // 2) + self.targetItem + selectItem for _ in range(self.fakeUserNum)]
        return sp.vstack([self.interact, fake_block(rows, self.fakeUserNum, self.itemNum)])
