// Stand-in: the reference includes this header and uses nothing from it.
#pragma once
