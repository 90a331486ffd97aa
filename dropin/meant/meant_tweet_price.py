"""`meant.meant_tweet_price` module path of the fork (src/meant/meant_tweet_price.py) -> native classes."""
from meant_amd.modules import *  # noqa: F401,F403
from meant_amd.modules import meantTweetPrice  # noqa: F401
