"""RandomAttack (reference attack/Black/RandomAttack.py:57-74): each fake user rates maliciousFeedbackNum random non-target fillers plus
every target.  The reference's default attack (conf/attack_parser.py)."""
import scipy.sparse as sp

from ._shilling import ShillingAttackModel, remaining_ids, filler_draw, fake_block


class RandomAttack(ShillingAttackModel):
    def posionDataAttack(self):
        pool = remaining_ids(self.itemNum, self.targetItem)
        rows = [filler_draw(pool, self.maliciousFeedbackNum) + self.targetItem for _ in range(self.fakeUserNum)]
        return sp.vstack([self.interact, fake_block(rows, self.fakeUserNum, self.itemNum)])
