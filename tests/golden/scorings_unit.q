bad_score          = X:-1000
fill_score         = -100

       A     C     G     T
A      1    -1    -1    -1
C     -1     1    -1    -1
G     -1    -1     1    -1
T     -1    -1    -1     1
